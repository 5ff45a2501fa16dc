"""Ragged buckets of dlrm_amd.graph.GraphedForward (lookup_capacity=...) on the GPU.  The oracle is the eager forward on the standard padded
batch (ragged_cases.padded: X padded with zero rows, offsets cat(off_req, full(bucket - n, nnz_k)), the request's own ids), compared on
rows < n as raw bits: right-aligning the ids inside the static buffers moves the bags, not what a lane sums."""
import numpy as np
import pytest
import torch

import ragged_cases as R
from ragged_cases import BATCH_SIZES, CAPACITY, EDGE_CASES, M_DEN, ROWS, T

pytestmark = pytest.mark.gpu

KINDS = (("fp32", 16), ("bf16", 16), ("q4", 16), ("qr", 16), ("md", 16), ("weighted", 16), ("fp32", 128))


def dev():
    return torch.device("cuda:0")


def make_model(kind, D=16):
    import dlrm_amd
    np.random.seed(3)
    F = T + 1
    ln_bot, ln_top = np.asarray([M_DEN, 8, D]), np.asarray([D + F * (F - 1) // 2, 8, 1])
    kw, m_spa = {}, D
    if kind == "qr":
        kw = dict(qr_flag=True, qr_operation="mult", qr_collisions=4, qr_threshold=100)
    if kind == "md":
        kw, m_spa = dict(md_flag=True, md_threshold=2), np.asarray([D, D // 4, D // 2])
    if kind == "weighted":
        kw = dict(weighted_pooling="learned")
    model = dlrm_amd.DLRM_Net(m_spa, np.asarray(ROWS), ln_bot, ln_top, "dot", sigmoid_top=1, loss_function="bce", **kw).to(dev())
    if kind == "weighted":                      # (the weights start as ones: give every row its own)
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            for w in model.v_W_l:
                w.copy_(torch.rand(w.shape, generator=g) + 0.5)
    if kind == "bf16":
        model.embedding_bfloat16()
    if kind == "q4":
        model.quantize_embedding(4)
    return model


def to_dev(req, stacked=False, shared=False):
    X, offs, ids = req
    X, offs, ids = X.to(dev()), [o.to(dev()) for o in offs], [i.to(dev()) for i in ids]
    if stacked:
        return X, torch.stack(offs), torch.stack(ids)
    if shared:
        return X, [offs[0]] * T, ids
    return X, offs, ids


def eager(model, X, lS_o, lS_i):
    with torch.no_grad():
        return model(X, lS_o, lS_i).clone()


def oracle(model, bucket, req, stacked=False):
    """rows < n of the eager forward on the padded batch"""
    assert bucket >= req[0].size(0)
    pad = R.padded(bucket, *req)
    assert R.well_formed(pad[1], pad[2], bucket)
    return eager(model, *to_dev(pad, stacked=stacked))[:req[0].size(0)]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))



def finish():
    from dlrm_amd import ops
    torch.cuda.synchronize()
    ops.check_index_errors(sync=True)


@pytest.mark.parametrize("kind,D", KINDS)
def test_every_kind_matches_eager_on_the_padded_batch(kind, D):
    """six requests of different (n, nnz) in the bucket of 8 — the edge cases: empty bags at the head, in the middle and at the end, n ==
    bucket with a non-empty last bag, nnz == Lcap (shift 0), a table without a lookup — then three in the bucket of 32: one eager call on the
    static buffers, ONE capture per bucket, every later request a replay"""
    from dlrm_amd.graph import GraphedForward
    model = make_model(kind, D)
    fwd = GraphedForward(model, batch_sizes=BATCH_SIZES, lookup_capacity=CAPACITY, warmup=1)
    for k, (name, n, lens) in enumerate(EDGE_CASES):
        req = R.make_request(n, 100 + k, lens=lens)
        Z = fwd(*to_dev(req))
        assert Z.shape == (n, 1)
        assert same_bits(Z, oracle(model, 8, req)), (kind, D, name)
    assert (fwd.captures, fwd.replays, fwd.exact_shapes, fwd.ragged_buckets_in_use) == (1, 5, 0, 1)
    assert fwd.staged_launches == 5             # X + 3 ids + 3 offsets segments: one stage_ragged_kernel launch per replay
    for k, n in enumerate((9, 32, 20)):
        req = R.make_request(n, 120 + k)
        assert same_bits(fwd(*to_dev(req)), oracle(model, 32, req)), (kind, D, n)
    assert (fwd.captures, fwd.exact_shapes, fwd.ragged_buckets_in_use, fwd.buckets_in_use) == (2, 0, 2, 2)
    finish()


def test_the_same_request_before_and_after_other_requests():
    """stale heads (longer requests leave ids in front of a shorter one's) and stale tails (rows n..) do not leak"""
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32")
    fwd = GraphedForward(model, batch_sizes=BATCH_SIZES, lookup_capacity=CAPACITY, warmup=1)
    mine = R.make_request(4, 200, lens=[[1, 0, 2, 1], [0, 0, 0, 3], [2, 2, 0, 0]])
    want = oracle(model, 8, mine)
    seen = []
    for k in range(7):
        if k % 2 == 0:
            seen.append(fwd(*to_dev(mine)).clone())
        else:
            other = R.make_request(8 if k == 3 else 6, 210 + k, lens=EDGE_CASES[2][2] if k == 3 else None)
            assert same_bits(fwd(*to_dev(other)), oracle(model, 8, other))
    assert len(seen) == 4 and all(same_bits(z, want) for z in seen)
    assert (fwd.captures, fwd.exact_shapes, fwd.ragged_buckets_in_use) == (1, 0, 1)
    finish()


@pytest.mark.parametrize("form", ("stacked_int32", "stacked_int64", "shared_offsets", "list_int32"))
def test_stacked_inputs_shared_offsets_and_int32(form):
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32")
    fwd = GraphedForward(model, batch_sizes=BATCH_SIZES, lookup_capacity=CAPACITY, warmup=1)
    idt = torch.int32 if form.endswith("int32") else torch.int64
    stacked, shared = form.startswith("stacked"), form == "shared_offsets"
    for k, n in enumerate((5, 8, 3, 7)):
        if shared:                              # one offsets tensor for all tables: the same bag lengths, every table its own ids
            lens = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(300 + k))
            req = R.make_request(n, 330 + k, lens=[lens] * T, idt=idt)
        else:
            req = R.make_request(n, 330 + k, idt=idt, same_nnz=stacked)
        args = to_dev(req, stacked=stacked, shared=shared)
        assert same_bits(fwd(*args), oracle(model, 8, req, stacked=stacked)), (form, k, n)
    assert (fwd.captures, fwd.replays, fwd.exact_shapes, fwd.ragged_buckets_in_use) == (1, 3, 0, 1)
    g = next(iter(fwd._buckets.values()))
    assert (g.plan.n_ids, g.plan.n_off) == ((T, 1) if shared else (T, T))
    finish()


def test_a_request_over_capacity_takes_an_exact_shape_graph():
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32")
    fwd = GraphedForward(model, batch_sizes=BATCH_SIZES, lookup_capacity=CAPACITY, warmup=1)
    lens = [[4, 3, 4, 3, 4, 3, 4, 3], [1, 0, 2, 1, 0, 1, 1, 1], [0, 1, 0, 1, 2, 2, 0, 0]]        # table 0: 28 lookups > Lcap = 24
    for s in range(3):
        req = to_dev(R.make_request(8, 400 + s, lens=lens))
        assert same_bits(fwd(*req), eager(model, *req)), s
    assert (fwd.captures, fwd.exact_shapes, fwd.ragged_buckets_in_use) == (1, 1, 0)
    fits = R.make_request(8, 410, lens=EDGE_CASES[1][2])                                            # ... and one that fits, next to it
    for _ in range(2):
        assert same_bits(fwd(*to_dev(fits)), oracle(model, 8, fits))
    assert (fwd.captures, fwd.exact_shapes, fwd.ragged_buckets_in_use) == (2, 1, 1)
    finish()


def test_capacity_one_at_d128_captures_the_two_kernel_form():
    """Lcap == bucket is the shape the fused lookup + interaction kernels take, and nnz == n does not prove one lookup per bag: an empty bag
    next to a two-lookup bag.  The ragged bucket states "not arange" for its static offsets, so the capture holds the two-kernel form."""
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32", 128)
    assert model.fuse_emb_interact is True
    fwd = GraphedForward(model, batch_sizes=BATCH_SIZES, lookup_capacity=1, warmup=1)
    for k, n in enumerate((8, 5, 8, 6)):
        lens = [[0, 2] + [1] * (n - 2), [1] * (n - 2) + [2, 0], [1, 0, 2] + [1] * (n - 3)]
        req = R.make_request(n, 500 + k, lens=lens)
        assert all(i.numel() == n for i in req[2])
        assert same_bits(fwd(*to_dev(req)), oracle(model, 8, req)), (k, n)
    assert (fwd.captures, fwd.exact_shapes, fwd.ragged_buckets_in_use) == (1, 0, 1) and model.fuse_emb_interact is True
    assert all(g.iota is False for g in fwd._buckets.values())
    for k in range(2):                          # one lookup per bag goes to the fixed-length bucket, as before
        X, offs, ids = R.make_request(8, 510 + k, lens=[[1] * 8] * T)
        assert same_bits(fwd(*to_dev((X, offs, ids))), eager(model, *to_dev((X, offs, ids))))
    assert fwd.ragged_buckets_in_use == 1 and fwd.buckets_in_use == 1 and len(fwd._buckets) == 2
    finish()


def test_a_bad_id_raises_once_at_the_next_call_and_the_id_buffers_are_zeroed():
    from dlrm_amd.graph import GraphedForward
    model = make_model("fp32")
    fwd = GraphedForward(model, batch_sizes=(8,), lookup_capacity=CAPACITY, warmup=1)
    for s in range(2):
        req = R.make_request(8, 600 + s)
        assert same_bits(fwd(*to_dev(req)), oracle(model, 8, req))
    X, offs, ids = R.make_request(8, 602, lens=EDGE_CASES[1][2])
    ids[1][3] = ROWS[1] + 5
    fwd(*to_dev((X, offs, ids)))
    torch.cuda.synchronize()
    small = R.make_request(2, 603, lens=[[1, 2], [0, 1], [3, 0]])
    with pytest.raises(IndexError, match="embedding index out of range: table 1, index %d, rows %d" % (ROWS[1] + 5, ROWS[1])):
        fwd(*to_dev(small))
    g = next(iter(fwd._buckets.values()))
    assert g.key[0] == "ragged" and all(int(t.abs().sum()) == 0 for t in g.static[2])
    for _ in range(2):
        assert same_bits(fwd(*to_dev(small)), oracle(model, 8, small))
    assert fwd.captures == 1
    finish()                                    # nothing left behind: the bad id is in front of no bag and in no buffer


def test_evaluate_inference_over_ragged_batches_equals_eager():
    """batches that fill their bucket (8 or 32 rows), every one with its own lookup counts: the padded batch IS the batch, so the graphed
    predictions are the eager ones bit for bit and every metric is equal"""
    from dlrm_amd import evaluate
    model = make_model("fp32")
    g = torch.Generator().manual_seed(9)
    batches, shapes = [], set()
    for k, n in enumerate((8, 8, 32, 8, 32, 8)):
        X, offs, ids = to_dev(R.make_request(n, 700 + k))
        shapes.add((n,) + tuple(i.numel() for i in ids))
        batches.append((X, offs, ids, torch.randint(0, 2, (n, 1), generator=g).float().to(dev())))
    assert len(shapes) == len(batches)
    want = evaluate.inference(model, batches)
    got = evaluate.inference(model, batches, graphed=True, batch_sizes=BATCH_SIZES, lookup_capacity=CAPACITY)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), k
    finish()
