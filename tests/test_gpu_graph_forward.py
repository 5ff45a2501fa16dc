"""dlrm_amd.graph.GraphedForward on the GPU: every model kind replayed bit-identically to its eager forward, buckets against the eager
forward on the padded batch, the offsets rule of the fused routes, staleness, bad ids and evaluate.inference(graphed=True)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [50, 120, 200]
T = len(ROWS)
M_DEN = 4
KINDS_16 = ("fp32", "bf16", "q8", "q4", "qr", "md", "mlp8", "mlp16", "q8_mlp16", "arith_bf16", "tr_dlrm", "tr_dcn", "tr_proj")
KINDS_128 = ("fp32", "bf16", "q8")          # the wide fused lookup + interaction routes


def dev():
    return torch.device("cuda:0")


def make_model(kind, D=16):
    import dlrm_amd
    from dlrm_amd.torchrec_variant import DLRM, DLRM_DCN, DLRM_Projection
    np.random.seed(3)
    F = T + 1
    ln_bot, ln_top = np.asarray([M_DEN, 8, D]), np.asarray([D + F * (F - 1) // 2, 8, 1])
    if kind == "tr_dlrm":
        return DLRM(ROWS, D, M_DEN, [8, D], [8, 1]).to(dev())
    if kind == "tr_dcn":
        return DLRM_DCN(ROWS, D, M_DEN, [8, D], [8, 1], dcn_num_layers=2, dcn_low_rank_dim=4).to(dev())
    if kind == "tr_proj":
        return DLRM_Projection(ROWS, D, M_DEN, [8, D], [8, 1], [8, D], [8, 2 * D]).to(dev())
    kw, m_spa = {}, D
    if kind == "qr":
        kw = dict(qr_flag=True, qr_operation="mult", qr_collisions=4, qr_threshold=100)
    if kind == "md":
        kw, m_spa = dict(md_flag=True, md_threshold=2), np.asarray([D, D // 4, D // 2])
    model = dlrm_amd.DLRM_Net(m_spa, np.asarray(ROWS), ln_bot, ln_top, "dot", sigmoid_top=1, loss_function="bce", **kw).to(dev())
    if kind == "bf16":
        model.embedding_bfloat16()
    if kind in ("q8", "q4", "q8_mlp16"):
        model.quantize_embedding(4 if kind == "q4" else 8)
    if kind in ("mlp8", "mlp16", "q8_mlp16"):
        model.quantize_mlp(8 if kind == "mlp8" else 16)
    if kind == "arith_bf16":
        model.set_mlp_arith("bf16")
    return model


def request(n, seed, stacked=False, P=1, idt=torch.int64):
    """one lookup (or P) per bag, fresh tensors every time: nobody vouches for the offsets"""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand((n, M_DEN), generator=g).to(dev())
    ids = [torch.randint(0, r, (n * P,), generator=g, dtype=torch.int64).to(idt).to(dev()) for r in ROWS]
    offs = [(torch.arange(n, dtype=idt) * P).to(dev()) for _ in ROWS]
    if stacked:
        return X, torch.stack(offs), torch.stack(ids)
    return X, offs, ids


def eager(model, X, lS_o, lS_i):
    with torch.no_grad():
        Z = model(X, lS_o, lS_i).clone()
    return Z


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _exact_shape_replays(kind, D):
    from dlrm_amd.graph import GraphedForward
    model = make_model(kind, D)
    fwd = GraphedForward(model, warmup=1)
    for s in range(4):                          # one eager call on the static buffers, the capture + first replay, two more replays
        req = request(8, 100 + s)
        Z = fwd(*req)
        assert Z.shape == (8, 1)
        assert same_bits(Z, eager(model, *req)), (kind, D, s)
    assert (fwd.captures, fwd.replays, fwd.exact_shapes) == (1, 3, 1)
    torch.cuda.synchronize()
    from dlrm_amd import ops
    ops.check_index_errors(sync=True)


@pytest.mark.parametrize("kind", KINDS_16)
def test_exact_shape_every_kind_d16(kind):
    _exact_shape_replays(kind, 16)


@pytest.mark.parametrize("kind", KINDS_128)
def test_exact_shape_fused_routes_d128(kind):
    _exact_shape_replays(kind, 128)


def test_list_inputs_take_the_staging_kernel_and_stacked_inputs_the_copies():
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32")
    fwd = GraphedForward(model, warmup=1)
    for s in range(3):
        req = request(8, 200 + s)
        assert same_bits(fwd(*req), eager(model, *req))
    assert fwd.replays == 2 and fwd.staged_launches == 2        # X + 3 offsets + 3 indices = 7 segments: one launch per replay
    for s in range(3):
        req = request(8, 210 + s, stacked=True, idt=torch.int32)
        assert same_bits(fwd(*req), eager(model, *req))
    assert fwd.replays == 4 and fwd.staged_launches == 2        # three tensors: hipMemcpyAsync each, no launch
    assert fwd.captures == 2 and fwd.exact_shapes == 2
    # a list that shares ONE offsets tensor among its tables is another structure (X + 1 + 3 segments)
    for s in range(3):
        X, offs, ids = request(8, 220 + s)
        req = (X, [offs[0]] * T, ids)
        assert same_bits(fwd(*req), eager(model, *req))
    assert fwd.captures == 3 and fwd.staged_launches == 4


class Padded:
    """what a bucket's static buffers hold: the oracle of a bucket is the eager forward on THIS batch"""

    def __init__(self, B, P=1):
        self.B, self.P = B, P
        self.X = torch.zeros((B, M_DEN), device=dev())
        self.ids = [torch.zeros(B * P, dtype=torch.int64, device=dev()) for _ in ROWS]

    def put(self, X, ids):
        n = X.size(0)
        self.X[:n] = X
        for d, s in zip(self.ids, ids):
            d[:n * self.P] = s

    def eager(self, model, n):
        offs = [torch.arange(self.B, dtype=torch.int64, device=dev()) * self.P for _ in ROWS]
        return eager(model, self.X.clone(), offs, [i.clone() for i in self.ids])[:n]


@pytest.mark.parametrize("kind,D", (("fp32", 16), ("q8_mlp16", 16), ("fp32", 128)))
def test_buckets_match_eager_on_the_padded_batch(kind, D):
    from dlrm_amd.graph import GraphedForward
    model = make_model(kind, D)
    fwd = GraphedForward(model, batch_sizes=(8, 32), warmup=1)
    pads = {8: Padded(8), 32: Padded(32)}
    five = None
    for k, n in enumerate((1, 5, 8, 9, 32, 5)):
        X, offs, ids = request(n, 300 if n == 5 else 301 + k)       # (the two n = 5 requests are the same request)
        pad = pads[8 if n <= 8 else 32]
        pad.put(X, ids)
        Z = fwd(X, offs, ids)
        assert Z.shape == (n, 1)
        assert same_bits(Z, pad.eager(model, n)), (kind, D, k, n)
        if n == 5:
            if five is None:
                five = Z.clone()
            else:
                assert same_bits(Z, five)       # other tail rows (the n = 8 request's), the same real rows
    assert fwd.captures == 2 and fwd.buckets_in_use == 2 and fwd.exact_shapes == 0
    assert fwd.replays == 4                     # one eager call per bucket in front of its capture


def test_bucket_boundary_ragged_and_fixed_length_requests():
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32")
    fwd = GraphedForward(model, batch_sizes=(8, 32), warmup=1)
    for s in range(2):                          # n above the largest bucket: an exact-shape graph
        req = request(33, 400 + s)
        assert same_bits(fwd(*req), eager(model, *req))
    assert (fwd.captures, fwd.exact_shapes, fwd.buckets_in_use) == (1, 1, 0)
    # a ragged multi-hot request: bags of 0 ... 3 lookups
    g = torch.Generator().manual_seed(5)
    for s in range(2):
        X = torch.rand((6, M_DEN), generator=g).to(dev())
        lens = [torch.tensor([0, 3, 1, 2, 0, 1]), torch.tensor([1, 1, 1, 1, 1, 2]), torch.tensor([2, 2, 2, 2, 2, 2])]
        lens[2][s] += 1                         # (table 2 would be a fixed P = 2 otherwise; the lookup counts stay the same per call shape)
        lens[2][5] -= 1
        offs = [(torch.cumsum(l, 0) - l).to(dev()) for l in lens]
        ids = [torch.randint(0, r, (int(l.sum()),), generator=g).to(dev()) for r, l in zip(ROWS, lens)]
        assert same_bits(fwd(X, offs, ids), eager(model, X, offs, ids))
    assert (fwd.captures, fwd.exact_shapes, fwd.buckets_in_use) == (2, 2, 0)
    # exactly two lookups in every bag: the bucket
    pad = Padded(8, P=2)
    for s in range(3):
        X, offs, ids = request(3 + s, 410 + s, P=2)
        pad.put(X, ids)
        assert same_bits(fwd(X, offs, ids), pad.eager(model, 3 + s))
    assert (fwd.captures, fwd.exact_shapes, fwd.buckets_in_use) == (3, 2, 1)


def test_offsets_that_are_not_arange_take_the_two_kernel_graph():
    """nnz == B without one lookup per bag: an empty bag next to a two-lookup bag.  The fused kernels would be wrong for it; the request's
    proof fails and the graph captured on its behalf holds the two-kernel form — the model's own switch is not touched."""
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32", 128)
    assert model.fuse_emb_interact is True
    fwd = GraphedForward(model, warmup=1)
    for s in range(3):
        X, offs, ids = request(8, 500 + s)
        offs = [torch.tensor([0, 0, 2, 3, 4, 5, 6, 7], device=dev()) for _ in ROWS]
        assert same_bits(fwd(X, offs, ids), eager(model, X, offs, ids))
    assert fwd.captures == 1 and model.fuse_emb_interact is True
    for s in range(3):                          # the same shapes with arange offsets: another graph, the fused kernels
        req = request(8, 510 + s)
        assert same_bits(fwd(*req), eager(model, *req))
    assert fwd.captures == 2 and fwd.exact_shapes == 2 and model.fuse_emb_interact is True
    X, offs, ids = request(8, 520)              # ... and back: the first graph is still there
    offs = [torch.tensor([0, 0, 2, 3, 4, 5, 6, 7], device=dev()) for _ in ROWS]
    assert same_bits(fwd(X, offs, ids), eager(model, X, offs, ids))
    assert fwd.captures == 2


def test_staleness_in_place_updates_moved_tables_and_invalidate():
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32")
    fwd = GraphedForward(model, warmup=1)
    req = request(8, 600)
    for _ in range(2):
        first = fwd(*req).clone()
    assert fwd.captures == 1
    # one eager SGD step between two replays: in place, visible in the next replay without a new capture
    opt = torch.optim.SGD(model.parameters(), lr=1.0)
    Xt, ot, it = request(8, 601)
    loss = model.loss_fn(model(Xt, ot, it), torch.ones((8, 1), device=dev()))
    opt.zero_grad()
    loss.backward()
    opt.step()
    del loss
    second = fwd(*req).clone()
    assert fwd.captures == 1
    assert same_bits(second, eager(model, *req)) and not same_bits(second, first)
    # the tables move (bfloat16 storage): the next call drops the graph, runs eagerly once, then captures again
    model.embedding_bfloat16()
    for _ in range(2):
        assert same_bits(fwd(*req), eager(model, *req))
    assert fwd.captures == 2 and fwd.exact_shapes == 1
    fwd.invalidate()
    assert fwd.exact_shapes == 0
    for _ in range(2):
        assert same_bits(fwd(*req), eager(model, *req))
    assert fwd.captures == 3


def test_bad_id_is_reported_at_the_next_call_and_does_not_stay_in_the_tail_rows():
    from dlrm_amd import ops
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32")
    fwd = GraphedForward(model, batch_sizes=(8,), warmup=1)
    pad = Padded(8)
    for s in range(2):
        X, offs, ids = request(8, 700 + s)
        pad.put(X, ids)
        assert same_bits(fwd(X, offs, ids), pad.eager(model, 8))
    X, offs, ids = request(8, 702)
    ids[1][6] = ROWS[1] + 5                     # row 6 of table 1: beyond a later, shorter request
    fwd(X, offs, ids)
    torch.cuda.synchronize()
    small = request(2, 703)
    with pytest.raises(IndexError, match="embedding index out of range: table 1, index %d, rows %d" % (ROWS[1] + 5, ROWS[1])):
        fwd(*small)
    clean = Padded(8)                           # the bucket's index rows went back to zero when the error surfaced
    clean.X.copy_(pad.X)
    clean.X[:8] = X
    clean.put(small[0], small[2])
    assert same_bits(fwd(*small), clean.eager(model, 2))
    torch.cuda.synchronize()
    ops.check_index_errors(sync=True)           # nothing left behind


def test_evaluate_inference_graphed_equals_eager():
    from dlrm_amd import evaluate
    model = make_model("fp32")
    g = torch.Generator().manual_seed(9)
    batches = []
    for k, n in enumerate((8, 8, 8, 3)):
        X, offs, ids = request(n, 800 + k)
        batches.append((X, offs, ids, torch.randint(0, 2, (n, 1), generator=g).float().to(dev())))
    want = evaluate.inference(model, batches)
    got = evaluate.inference(model, batches, graphed=True)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), k


@pytest.mark.parametrize("order", ((8, 5, 8, 3, 5), (5, 8, 3, 8, 1)))
def test_stacked_requests_in_a_bucket_whatever_the_first_one_was(order):
    """the bucket's staging plan is built from its first request: one that fills the bucket and one that does not must both leave a
    plan that puts the T rows of a narrower [T, n] request at the heads of the T rows of the static [T, bucket] buffer"""
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32")
    fwd = GraphedForward(model, batch_sizes=(8,), warmup=1)
    pad = Padded(8)
    for k, n in enumerate(order):
        X, offs, ids = request(n, 900 + k, stacked=True)
        assert ids.shape == (T, n)
        pad.put(X, ids)
        Z = fwd(X, offs, ids)
        assert Z.shape == (n, 1) and same_bits(Z, pad.eager(model, n)), (order, k, n)
    assert fwd.captures == 1 and fwd.buckets_in_use == 1 and fwd.replays == len(order) - 1
    # every request, one that fills the bucket included, is X + T rows = 4 segments: at the threshold, so copies and no staging launch
    assert fwd._buckets and all(g.plan.n == 1 + T for g in fwd._buckets.values()) and fwd.staged_launches == 0
    # ... and the same requests through the staging kernel
    fwd.stage_memcpy_max = 0
    for k, n in enumerate(order):
        X, offs, ids = request(n, 950 + k, stacked=True)
        pad.put(X, ids)
        assert same_bits(fwd(X, offs, ids), pad.eager(model, n)), (order, k, n)
    assert fwd.staged_launches == len(order) and fwd.captures == 1
    torch.cuda.synchronize()
    from dlrm_amd import ops
    ops.check_index_errors(sync=True)


def test_one_bad_request_raises_once_even_when_the_next_request_is_replayed_before_it_is_seen():
    """no synchronisation between the bad request and the next, shorter one: if the report is not in yet, that request is replayed with the
    bad id still in the bucket's tail rows and reports it a second time.  Exactly one call raises; the requests after it are clean."""
    from dlrm_amd import ops
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32")
    fwd = GraphedForward(model, batch_sizes=(8,), warmup=1)
    for s in range(2):
        fwd(*request(8, 1000 + s))
    X, offs, ids = request(8, 1002)
    ids[1][6] = ROWS[1] + 5
    fwd(X, offs, ids)
    raised = 0
    try:
        fwd(*request(2, 1003))                  # no wait in between: replayed over the bad row, or the report is in already and it raises
    except IndexError:
        raised += 1
    torch.cuda.synchronize()
    pad = Padded(8)                             # after the raise the index rows are zero; rows 2.. of X keep the bad request's
    pad.X[:8] = X
    for s in range(3):
        small = request(2, 1010 + s)
        try:
            Z = fwd(*small)
        except IndexError:
            raised += 1
            assert s == 0                       # only the call right after can still answer for the bad request
            Z = fwd(*small)
        assert raised == 1                      # (by now the report has been seen, by one call or the other)
        pad.put(small[0], small[2])
        assert same_bits(Z, pad.eager(model, 2)), s
        torch.cuda.synchronize()
    assert raised == 1
    ops.check_index_errors(sync=True)


def test_the_verdict_on_the_static_offsets_survives_an_emptied_proof_cache():
    """iota.py drops its per-object verdicts wholesale when many other tensors were proven; the two-kernel graph of a request whose
    offsets are not arange must still be captured as the two-kernel form (undecided offsets under capture would take the fused kernels)"""
    from dlrm_amd import iota
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32", 128)
    fwd = GraphedForward(model, warmup=1)
    for s in range(3):
        X, offs, ids = request(8, 1100 + s)
        offs = [torch.tensor([0, 0, 2, 3, 4, 5, 6, 7], device=dev()) for _ in ROWS]
        want = eager(model, X, offs, ids)
        iota._iota_cache.clear()                # (between the graph's creation, its eager call and its capture)
        assert same_bits(fwd(X, offs, ids), want), s
    assert fwd.captures == 1 and fwd.replays == 2
