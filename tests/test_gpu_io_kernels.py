"""The evaluation metrics, the synthetic batch generator, the Criteo record transform, the multi-hot expansion and table generator, the block
copies / column padding and the dense optimizer updates (csrc/metrics.hip, datagen.hip, multihot.hip, loss_opt.hip, adagrad.hip) against the
oracle functions of oracle/oracle.py and the exact restatements of tests/test_io_kernels_host.py.

Shapes are the smallest that reach each path: one element, one block of 256 and its neighbours, a grid-stride loop that wraps its capped grid,
more operands than one launch group takes, the compiled limits and the refusal just above them, operands one float off a 16-byte boundary.
Every output and workspace handed to a kernel lies inside a larger buffer filled with a canary, which must be intact afterwards.  Kernels run
with valid arguments only, or with arguments the entry point refuses before it launches anything."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_io_kernels_host as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

E_ARG, E_ALIGN, E_RANGE, E_MODE = -1, -2, -3, -4
CANARY_F = np.array([0xDEADBEEF], dtype=np.uint32).view(np.float32)[0]      # a finite, unmistakable fp32 bit pattern
CANARY_I = -0x5A5A5A5B


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(dev())


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def lib_and_stream():
    from dlrm_amd import _lib
    return _lib.load(), C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def f32_canary(shape):
    return torch.full(shape, float(CANARY_F), dtype=torch.float32, device=dev())


def f32_bits_equal(t, bits):
    """every element of the fp32 tensor t carries the bit pattern `bits`"""
    return bool((t.contiguous().view(torch.int32) == int(np.uint32(bits).astype(np.int32))).all())


def canary_intact(t):
    return f32_bits_equal(t, CANARY_F.view(np.uint32))


def guarded_f32(a, k=0, guard=8):
    """1-D fp32 numpy `a` on the device as a view that starts guard + k elements into a canary-filled buffer (the buffer's start is at least
    256-byte aligned and guard is a multiple of 4: k = 1 puts the view one float off a 16-byte boundary).  Returns (view, buffer)."""
    buf = f32_canary((a.size + 2 * guard + 4,))
    v = buf[guard + k:guard + k + a.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() % 16 == (4 * k) % 16
    return v, buf


def guards_intact(buf, v):
    lo = (v.data_ptr() - buf.data_ptr()) // 4
    return canary_intact(buf[:lo]) and canary_intact(buf[lo + v.numel():])


# ================================================================================================ 1. dlrm_binary_metrics
WS_GUARD = 1024


def metrics_guarded(s, t, short=0, shift=0):
    """dlrm_binary_metrics through ctypes: the workspace of dlrm_binary_metrics_workspace_bytes(n) bytes sits between two canary regions, the
    9 doubles in front of 7 canary doubles.  Returns (rc, out float64 [9] on the host, guards intact, out untouched)."""
    lib, st = lib_and_stream()
    n = s.size
    need = int(lib.dlrm_binary_metrics_workspace_bytes(n))
    assert need > 0 and need % 256 == 0
    ws = torch.full((need + 2 * WS_GUARD,), 0xA5, dtype=torch.uint8, device=dev())
    out = torch.full((16,), -12345.6789, dtype=torch.float64, device=dev())
    ts, tt = to_dev(s), to_dev(t)
    rc = lib.dlrm_binary_metrics(n, ptr(ts), ptr(tt), ptr(out), ptr(ws, WS_GUARD + shift), need - short, st)
    torch.cuda.synchronize()
    guards = bool((ws[:WS_GUARD] == 0xA5).all()) and bool((ws[WS_GUARD + need:] == 0xA5).all()) and bool((out[9:] == -12345.6789).all())
    return rc, out[:9].cpu().numpy(), guards, bool((out == -12345.6789).all())


def check_metrics(got9, s, t):
    o = O.binary_metrics(s, t)
    got = dict(zip(("n", "positives", "tp", "fp", "fn", "tn", "roc_auc", "ap", "round_matches"), got9.tolist()))
    for k in H.COUNTERS:
        assert got[k] == o[k], (k, got[k], o[k])
    if np.isnan(o["roc_auc"]):
        assert np.isnan(got["roc_auc"])
    else:
        assert got["roc_auc"] == o["roc_auc"], (got["roc_auc"], o["roc_auc"], got["roc_auc"] - o["roc_auc"])
    if np.isnan(o["ap"]):
        assert np.isnan(got["ap"])
    else:
        G = H.distinct_scores(s)
        print("ap: got %.17g ref %.17g |diff| %.3g bound %.3g (G = %d)" % (got["ap"], o["ap"], abs(got["ap"] - o["ap"]), H.ap_bound(G, o["ap"]), G))
        assert abs(got["ap"] - o["ap"]) <= H.ap_bound(G, o["ap"]), (got["ap"], o["ap"], G)
    return got, o


@pytest.mark.parametrize("n", H.METRIC_SIZES)
@pytest.mark.parametrize("family", H.METRIC_FAMILIES)
def test_binary_metrics_counters_auc_ap_order_and_guards(family, n):
    """Counters exact.  roc_auc BIT-EQUAL to O.binary_metrics: each trapezoid term d_fp (tp + tp_prev) 0.5 is an exact multiple of 0.5, every
    partial sum is bounded by P N < 2^53 (n <= 2^26), so the fp64 sum is exact in any order on both sides; one division of the same two exact
    numbers follows.  ap within 2 (G + 2) 2^-53 ref, G = number of distinct scores (H.ap_bound).  A random permutation of the same (score,
    target) pairs, and a second call (through ops.binary_metrics_raw), return the same 9 doubles bit for bit: the header's "deterministic,
    fixed reduction order".  The workspace and the output are not overrun."""
    from dlrm_amd import ops
    s, t = H.metric_case(family, n)
    rc, got9, guards, _ = metrics_guarded(s, t)
    assert rc == 0 and guards
    got, o = check_metrics(got9, s, t)
    again = ops.binary_metrics_raw(to_dev(s), to_dev(t)).cpu().numpy()
    assert np.array_equal(bits64(again), bits64(got9))
    p = np.random.default_rng(n).permutation(n)
    rc, perm9, guards, _ = metrics_guarded(s[p], t[p])
    assert rc == 0 and guards and np.array_equal(bits64(perm9), bits64(got9)), (perm9, got9)
    if family == "edges" and n >= 255:
        assert got["round_matches"] < n and got["tp"] + got["fp"] > got["round_matches"]     # scores >= 1.5 predict 1 and never match


@pytest.mark.parametrize("n", H.METRIC_SIZES)
def test_binary_metrics_degenerate_targets(n):
    """all targets 1: roc_auc NaN and ap == 1.0 exactly; all 0: both NaN and recall = precision = f1 = 0; n == 1 with either target"""
    from dlrm_amd import ops
    s, _ = H.metric_case("logits", n)
    ones, zeros = np.ones(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    rc, g1, guards, _ = metrics_guarded(s, ones)
    assert rc == 0 and guards
    check_metrics(g1, s, ones)
    assert np.isnan(g1[6]) and g1[7] == 1.0 and g1[1] == n
    rc, g0, guards, _ = metrics_guarded(s, zeros)
    assert rc == 0 and guards
    check_metrics(g0, s, zeros)
    assert np.isnan(g0[6]) and np.isnan(g0[7]) and g0[1] == 0
    m = ops.binary_metrics(to_dev(s), to_dev(zeros))
    assert m["recall"] == 0.0 and m["precision"] == 0.0 and m["f1"] == 0.0 and np.isnan(m["roc_auc"]) and np.isnan(m["ap"])
    m = ops.binary_metrics(to_dev(s), to_dev(ones))
    assert np.isnan(m["roc_auc"]) and m["ap"] == 1.0


@pytest.mark.parametrize("n", [1, 257])
def test_binary_metrics_refuses_short_or_misaligned_workspace(n):
    s, t = H.metric_case("k3", n)
    rc, _, guards, untouched = metrics_guarded(s, t, short=1)
    assert rc == E_ARG and guards and untouched
    rc, _, guards, untouched = metrics_guarded(s, t, shift=8)
    assert rc == E_ALIGN and guards and untouched


# ================================================================================================ 2. generator and Criteo transform
GEN_ROWS = [1, 2, 3, 129, 1000, 2 ** 31]
GEN_CASES = [(2, 257), (3, 1), (3, 255), (3, 256), (3, 257), (127, 257), (128, 257)]
TORCH_INT = {torch.int32: np.int32, torch.int64: np.int64}


def gen_bags_guarded(rows, B, P, fixed, seed, dtype, guard=5):
    """dlrm_gen_uniform_bags through ctypes with buffers of this test: per table a row of B offsets and B * P index slots, `guard` canary slots
    after each.  Returns (rc, off [T, B + guard], idx [T, B P + guard], nnz [T + guard]) on the host."""
    from dlrm_amd import _lib
    lib, st = lib_and_stream()
    T = len(rows)
    slots = B * max(P, 1)
    off = torch.full((T, B + guard), CANARY_I, dtype=dtype, device=dev())
    idx = torch.full((T, slots + guard), CANARY_I, dtype=dtype, device=dev())
    nnz = torch.full((T + guard,), CANARY_I, dtype=torch.int64, device=dev())
    need = max(int(lib.dlrm_gen_workspace_bytes(T, B)), 256)
    ws = torch.full((need + 1024,), 0xA5, dtype=torch.uint8, device=dev())
    rc = lib.dlrm_gen_uniform_bags(T, B, _lib.i64_array(rows), P, int(fixed), seed, 64 if dtype == torch.int64 else 32,
                                   _lib.ptr_array([off[k].data_ptr() for k in range(T)]), _lib.ptr_array([idx[k].data_ptr() for k in range(T)]),
                                   ptr(nnz), ptr(ws), need, st)
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all())
    return rc, off.cpu().numpy(), idx.cpu().numpy(), nnz.cpu().numpy()


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("P,B", GEN_CASES)
def test_generator_bit_exact_at_the_lookup_limit_and_block_edges(P, B, fixed, idx_dtype):
    """UniformBatchGenerator.batch against O.philox_bags / O.philox_dense, bit for bit: even P, odd P (half a Philox block unused), the compiled
    limit 128 and one below; one bag, one block of 256 bags and its neighbours; tables of 1, 2, 3 rows under a large P, and of 2^31 rows (ids
    up to 2^31 - 1, the largest an int32 holds).  The same entry point with this test's buffers: nothing is written after a table's nnz
    indices or after its B offsets."""
    from dlrm_amd.datagen import UniformBatchGenerator
    gen = UniformBatchGenerator(13, GEN_ROWS, P, fixed, round_targets=True, seed=11, device=dev(), index_dtype=idx_dtype)
    X, lS_o, lS_i, T = gen.batch(B, batch_no=2)
    torch.cuda.synchronize()
    assert np.array_equal(bits32(X.cpu().numpy().reshape(-1)), bits32(O.philox_dense(B * 13, gen._seed(2, 1))))
    assert np.array_equal(bits32(T.cpu().numpy().reshape(-1)), bits32(O.philox_dense(B, gen._seed(2, 2), round_values=True)))
    rc, off_g, idx_g, nnz_g = gen_bags_guarded(GEN_ROWS, B, P, fixed, gen._seed(2, 16), idx_dtype)
    assert rc == 0 and np.all(nnz_g[len(GEN_ROWS):] == CANARY_I)
    for t, n in enumerate(GEN_ROWS):
        off, idx = O.philox_bags(t, n, B, P, fixed, gen._seed(2, 16))
        assert lS_o[t].dtype == idx_dtype and lS_i[t].dtype == idx_dtype
        assert np.array_equal(lS_o[t].cpu().numpy().astype(np.int64), off), t
        assert np.array_equal(lS_i[t].cpu().numpy().astype(np.int64), idx), t
        assert nnz_g[t] == idx.size and np.array_equal(off_g[t, :B].astype(np.int64), off) and np.array_equal(idx_g[t, :idx.size].astype(np.int64), idx)
        assert np.all(off_g[t, B:] == CANARY_I) and np.all(idx_g[t, idx.size:] == CANARY_I), t
        if n == 1:
            assert np.array_equal(off, np.arange(B)) and not idx.any()               # every bag is [0]
        if n == 2 and P == 128 and fixed:
            bags = np.split(lS_i[t].cpu().numpy(), off[1:])
            assert all(list(b) in ([0], [1], [0, 1]) for b in bags) and any(len(b) == 2 for b in bags)
        if n == 2 ** 31 and B >= 255:
            assert idx.max() > 2 ** 30 and idx.max() <= 2 ** 31 - 1 and lS_i[t].min() >= 0


@pytest.mark.parametrize("P", [129, 0])
def test_generator_refuses_lookups_beyond_the_compiled_limit(P):
    """P = 129 (kMaxLookups + 1) and P = 0: the entry point returns DLRM_E_RANGE before it launches, nothing is written; the generator raises"""
    from dlrm_amd.datagen import UniformBatchGenerator
    rc, off, idx, nnz = gen_bags_guarded([1000, 3], 67, P, False, 5, torch.int64)
    assert rc == E_RANGE and np.all(off == CANARY_I) and np.all(idx == CANARY_I) and np.all(nnz == CANARY_I)
    gen = UniformBatchGenerator(4, [1000, 3], P, False, device=dev())
    with pytest.raises(RuntimeError, match="DLRM_E_RANGE"):
        gen.batch(67)


def test_generator_35_tables_cross_a_launch_group_with_a_seed_per_group():
    """table t = O.philox_bags(t % 32, rows[t], ..., seed of launch group t // 32): tables 0 and 32 have equal rows and must differ"""
    from dlrm_amd.datagen import UniformBatchGenerator
    rng = np.random.default_rng(35)
    rows = [int(v) for v in rng.choice([1, 2, 3, 7, 129, 1000, 39884406], size=35)]
    rows[0] = rows[32] = 1000
    B, P = 67, 3
    for idx_dtype in (torch.int64, torch.int32):
        gen = UniformBatchGenerator(4, rows, P, False, seed=3, device=dev(), index_dtype=idx_dtype)
        _, lS_o, lS_i, _ = gen.batch(B, batch_no=9)
        torch.cuda.synchronize()
        assert len(lS_o) == 35 and len(lS_i) == 35
        for t, n in enumerate(rows):
            off, idx = O.philox_bags(t % 32, n, B, P, False, gen._seed(9, 16 + 32 * (t // 32)))
            assert np.array_equal(lS_o[t].cpu().numpy().astype(np.int64), off), t
            assert np.array_equal(lS_i[t].cpu().numpy().astype(np.int64), idx), t
        assert not (lS_i[0].numel() == lS_i[32].numel() and torch.equal(lS_i[0], lS_i[32]))


def test_generator_refuses_int32_ids_for_a_table_beyond_2_to_31_rows():
    from dlrm_amd.datagen import UniformBatchGenerator
    with pytest.raises(RuntimeError, match="int32"):
        UniformBatchGenerator(4, [10, 2 ** 31 + 1], 2, True, device=dev(), index_dtype=torch.int32)
    UniformBatchGenerator(4, [10, 2 ** 31 + 1], 2, True, device=dev(), index_dtype=torch.int64)
    gen = UniformBatchGenerator(4, [2 ** 31], 1, True, seed=1, device=dev(), index_dtype=torch.int32)     # the one-hot kernel at the largest table
    _, lS_o, lS_i, _ = gen.batch(300, 0)
    assert np.array_equal(lS_i[0].cpu().numpy().astype(np.int64), O.philox_onehot(0, 2 ** 31, 300, gen._seed(0, 16)))
    assert int(lS_i[0].max()) > 2 ** 30 and int(lS_i[0].min()) >= 0


@pytest.mark.parametrize("round_values", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 511, 513])
def test_gen_uniform_dense_bit_exact_and_stops_at_n(n, round_values):
    """two values per thread: with n odd the last thread's second value must not be stored (a canary follows x[n-1])"""
    lib, st = lib_and_stream()
    buf = f32_canary((n + 16,))
    x = buf[8:8 + n]
    assert lib.dlrm_gen_uniform_dense(n, ptr(x), int(round_values), 0x123456789ABCDEF, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits32(x.cpu().numpy()), bits32(O.philox_dense(n, 0x123456789ABCDEF, round_values)))
    assert guards_intact(buf, x)


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("B", H.CRITEO_B)
def test_criteo_bin_transform_edges_of_counts_ids_and_tile(B, idx_dtype):
    """dlrm_criteo_bin_transform on synthetic raw records (H.criteo_raw), ldx = 16 and ld_idx = B + 3 with canary columns, for every
    max_ind_range of H.CRITEO_RANGES: ids / offsets / targets bit-exact against O.criteo_bin_transform (python's % of negative ids; with
    max_ind_range <= 0 negative ids pass through unchanged); X has -inf where the count is -1 and NaN where it is below, in the oracle's
    positions, and elsewhere lies within ONE fp32 ulp (a bit distance) of the correctly rounded log(float32(count) + 1)."""
    lib, st = lib_and_stream()
    for mir in H.CRITEO_RANGES:
        raw = H.criteo_raw(B, mir)
        with np.errstate(divide="ignore", invalid="ignore"):                 # counts -1 and -2: log 0 and log of a negative, on purpose
            Xr, lS_o, lS_i, Tr = O.criteo_bin_transform(raw, mir)
        X = f32_canary((B, 16))
        idx = torch.full((26, B + 3), CANARY_I, dtype=idx_dtype, device=dev())
        off = torch.full((26, B + 3), CANARY_I, dtype=idx_dtype, device=dev())
        tgt = f32_canary((B + 4,))
        traw = to_dev(raw)
        rc = lib.dlrm_criteo_bin_transform(B, ptr(traw), mir, 64 if idx_dtype == torch.int64 else 32, ptr(X), 16, ptr(idx), ptr(off),
                                           B + 3, ptr(tgt), st)
        torch.cuda.synchronize()
        assert rc == 0
        assert canary_intact(X[:, 13:]) and canary_intact(tgt[B:]) and bool((idx[:, B:] == CANARY_I).all()) and bool((off[:, B:] == CANARY_I).all())
        assert np.array_equal(idx[:, :B].cpu().numpy().astype(np.int64), lS_i), (mir, "ids")
        assert np.array_equal(off[:, :B].cpu().numpy().astype(np.int64), lS_o)
        assert np.array_equal(bits32(tgt[:B].cpu().numpy()), bits32(Tr.reshape(-1)))
        if mir <= 0 and idx_dtype == torch.int32:
            assert np.array_equal(idx[:, :B].cpu().numpy(), raw[:, 14:].T) and int(idx[:, :B].min()) == H.INT32_MIN
        got = X[:, :13].cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(Xr)) and np.array_equal(np.isneginf(got), np.isneginf(Xr)) and not np.isposinf(got).any()
        assert np.isnan(got).sum() >= B and np.isneginf(got).sum() >= B
        fin = np.isfinite(Xr)
        d = H.ulp_distance32(got[fin], H.criteo_log_ref(raw)[fin])
        assert int(d.max()) <= 1, (mir, int(d.max()))


# ================================================================================================ 3. multi-hot expansion and tables
def expand_guarded(mh, ids, want_global=True, guard=64):
    """dlrm_multihot_expand through ctypes on the uploaded tables of `mh` (`multi_hot_tables_l`), values / offsets inside canary-filled
    buffers; the index-error block {flag, table, index, rows} is this test's own and must stay clear (every id is in range)"""
    from dlrm_amd import _lib
    lib, st = lib_and_stream()
    tabs = mh.multi_hot_tables_l
    T = len(tabs)
    B = ids.size(1)
    nv = B * sum(int(t.size(1)) for t in tabs)
    values = torch.full((nv + guard,), CANARY_I, dtype=torch.int32, device=dev())
    off_g = torch.full((T * B + 1 + guard,), CANARY_I, dtype=torch.int64, device=dev())
    off_l = torch.full((T * B + guard,), CANARY_I, dtype=torch.int32, device=dev())
    err = torch.zeros(8, dtype=torch.int64, device=dev())
    rc = lib.dlrm_multihot_expand(T, B, ptr(ids), 64 if ids.dtype == torch.int64 else 32, _lib.ptr_array([t.data_ptr() for t in tabs]),
                                  _lib.i64_array([t.size(0) for t in tabs]), (C.c_int * T)(*[int(t.size(1)) for t in tabs]), ptr(values),
                                  ptr(off_g) if want_global else None, ptr(off_l), ptr(err), st)
    torch.cuda.synchronize()
    assert rc == 0 and not bool(err.any())
    assert bool((values[nv:] == CANARY_I).all()) and bool((off_l[T * B:] == CANARY_I).all())
    assert bool((off_g[T * B + 1 if want_global else 0:] == CANARY_I).all())
    return values[:nv].cpu().numpy(), off_g[:T * B + 1].cpu().numpy(), off_l[:T * B].cpu().numpy().reshape(T, B)


def check_expand(tabs, B, id_dtype, seed):
    from dlrm_amd import ops
    from dlrm_amd.multihot import Multihot
    rng = np.random.default_rng(seed)
    T = len(tabs)
    ids = np.stack([rng.integers(0, tab.shape[0], size=B) for tab in tabs])
    ids[:, 0] = 0
    ids[:, -1] = [tab.shape[0] - 1 for tab in tabs]
    want_v, want_o = O.multihot_expand(ids, tabs)
    want_l = np.stack([np.arange(B) * tab.shape[1] for tab in tabs])
    mh = Multihot.from_host_tables(tabs, B, device=dev())
    tid = to_dev(ids).to(id_dtype)
    v, og, ol = expand_guarded(mh, tid)
    assert np.array_equal(v, want_v) and np.array_equal(og, want_o) and og[-1] == want_v.size and np.array_equal(ol, want_l)
    v, _, ol = expand_guarded(mh, tid, want_global=False)
    assert np.array_equal(v, want_v) and np.array_equal(ol, want_l)
    values, off_g, off_l = mh.expand(tid)
    assert values.dtype == torch.int32 and off_g.dtype == torch.int64 and off_l.dtype == torch.int32
    assert np.array_equal(values.cpu().numpy(), want_v) and np.array_equal(off_g.cpu().numpy(), want_o) and np.array_equal(off_l.cpu().numpy(), want_l)
    values, off_g, off_l2 = mh.expand(tid, want_global_offsets=False)
    assert off_g is None and np.array_equal(values.cpu().numpy(), want_v) and np.array_equal(off_l2.cpu().numpy(), want_l)
    ops.check_index_errors(sync=True)
    return mh, off_l


def random_tables(rng, hots, rows):
    return [rng.integers(H.INT32_MIN, H.INT32_MAX + 1, size=(n, h)).astype(np.int32) for n, h in zip(rows, hots)]


@pytest.mark.parametrize("id_dtype", [torch.int64, torch.int32])
def test_multihot_expand_35_tables_cross_a_launch_group(id_dtype):
    """35 tables (32 + 3), hot sizes from {1, 2, 3, 7}, rows from {1, 3, 50, 1000}, B = 67, random int32 contents: values, global offsets (with
    the final element T B ... = the number of values) and local offsets bit-exact against O.multihot_expand"""
    rng = np.random.default_rng(3)
    hots = [int(v) for v in rng.choice([1, 2, 3, 7], size=35)]
    rows = [int(v) for v in rng.choice([1, 3, 50, 1000], size=35)]
    hots[31], hots[32], hots[34] = 7, 2, 3                    # the group boundary and the last table are not 1-hot
    check_expand(random_tables(rng, hots, rows), 67, id_dtype, 4)


def test_multihot_expand_wraps_the_4096_block_grid():
    """a 256-hot table next to a 1-hot one at B = 4100: B h = 1049600 > 4096 * 256 elements, the grid-stride loop takes a second trip"""
    rng = np.random.default_rng(5)
    check_expand(random_tables(rng, [256, 1], [50, 50]), 4100, torch.int64, 6)


def test_multihot_expand_all_one_hot_is_marked_one_lookup_per_bag():
    from dlrm_amd import iota, ops
    rng = np.random.default_rng(7)
    mh, off_l = check_expand(random_tables(rng, [1, 1, 1], [1, 3, 50]), 67, torch.int32, 8)
    assert np.array_equal(off_l.cpu().numpy(), np.tile(np.arange(67), (3, 1)))
    before = iota.IOTA_STATS["tagged"]
    assert ops.offsets_are_iota(off_l) is True and iota.IOTA_STATS["tagged"] == before + 1       # the producer's tag, no device pass
    _, off_l7 = check_expand(random_tables(rng, [1, 2], [3, 3]), 67, torch.int32, 9)
    assert not iota._iota_tagged(off_l7) and ops.offsets_are_iota(off_l7) is False


BIG_HOT, BIG_ROWS, BIG_SEED = 8, 2097277, 77                # rows * hot = 65536 * 256 + 1000: the table generator's grid cap is crossed by 1000
assert BIG_HOT * BIG_ROWS == 65536 * 256 + 1000


@pytest.fixture(scope="module")
def big_table():
    from dlrm_amd.multihot import Multihot
    mh = Multihot([1, BIG_HOT], [3, BIG_ROWS], 16, dist_type="uniform", device=dev(), seed=BIG_SEED)
    torch.cuda.synchronize()
    return mh.multi_hot_tables_l[1]


@pytest.mark.parametrize("where", ["first", "wrap", "last"])
def test_multihot_generated_table_across_the_65536_block_cap(big_table, where):
    """rows at the start, around flat element 65536 * 256 (where the grid-stride loop wraps) and at the end, bit-exact against the row-range
    restatement H.multihot_uniform_rows (pinned on the CPU to O.philox_multihot_table); column 0 = arange and 0 <= value < rows everywhere"""
    wrap_row = 65536 * 256 // BIG_HOT
    r0 = {"first": 0, "wrap": wrap_row - 500, "last": BIG_ROWS - 1000}[where]
    r1 = min(r0 + 1000, BIG_ROWS)                           # the wrap lies 125 rows before the end: its window stops there
    got = big_table[r0:r1].cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (r1 - r0, BIG_HOT)
    assert np.array_equal(got, H.multihot_uniform_rows(1, BIG_ROWS, BIG_HOT, BIG_SEED, r0, r1))
    if where == "first":
        assert torch.equal(big_table[:, 0], torch.arange(BIG_ROWS, dtype=torch.int32, device=dev()))
        assert int(big_table.min()) >= 0 and int(big_table.max()) < BIG_ROWS and int(big_table[:, 1:].max()) > BIG_ROWS - 100


def test_multihot_gen_table_refusals():
    lib, st = lib_and_stream()
    out = torch.full((64 + 16,), CANARY_I, dtype=torch.int32, device=dev())
    assert lib.dlrm_multihot_gen_table(0, 2 ** 31, 1, 0, 1, ptr(out), st) == E_ARG          # ids are int32: rows must stay below 2^31
    assert lib.dlrm_multihot_gen_table(0, 8, 8, 2, 1, ptr(out), st) == E_MODE               # dist 2 does not exist
    torch.cuda.synchronize()
    assert bool((out == CANARY_I).all())
    assert lib.dlrm_multihot_gen_table(0, 8, 8, 0, 1, ptr(out), st) == 0                     # and the same call with dist 0 does run
    torch.cuda.synchronize()
    assert np.array_equal(out[:64].cpu().numpy().reshape(8, 8), O.philox_multihot_table(0, 8, 8, 0, 1)) and bool((out[64:] == CANARY_I).all())


# ================================================================================================ 4. block copies and padding
def layout(widths, gap, align4_every=None):
    """column start of every block in one row-major matrix with `gap` free columns between blocks; returns (starts, total columns)"""
    starts, o = [], gap
    for k, w in enumerate(widths):
        if align4_every and k % align4_every == 0:
            o = (o + 3) // 4 * 4
        starts.append(o)
        o += w + gap
    return starts, o


def run_copy_blocks(M, widths, src_ld_extra, dst_ld, seed, first_src_off_by_one=False, align4_every=None):
    from dlrm_amd import ops
    rng = np.random.default_rng(seed)
    s_starts, s_cols = layout(widths, 2, align4_every)
    d_starts, d_cols = layout(widths, 3, align4_every)
    s_ld = (s_cols + 3) // 4 * 4 + src_ld_extra
    d_ld = max(dst_ld or 0, (d_cols + 3) // 4 * 4)
    src_np = H.random_bits_f32(rng, (M, s_ld))
    src = to_dev(src_np)
    dst = f32_canary((M, d_ld))
    srcs = [src[:, a:a + w] for a, w in zip(s_starts, widths)]
    if first_src_off_by_one:                                 # a contiguous [M, w0] block that starts one float into its allocation
        flat = to_dev(np.concatenate([H.random_bits_f32(rng, (1,)), src_np[:, s_starts[0]:s_starts[0] + widths[0]].reshape(-1)]))
        srcs[0] = flat[1:].view(M, widths[0])
        assert srcs[0].data_ptr() % 16 == 4
    dsts = [dst[:, a:a + w] for a, w in zip(d_starts, widths)]
    ops.copy_blocks(srcs, dsts)
    torch.cuda.synchronize()
    want = np.full((M, d_ld), CANARY_F, dtype=np.float32)
    for a, b, w in zip(s_starts, d_starts, widths):
        want[:, b:b + w] = src_np[:, a:a + w]
    assert np.array_equal(bits32(dst.cpu().numpy()), bits32(want))
    return srcs, dsts


def test_copy_blocks_70_blocks_cross_a_launch_group():
    """70 blocks (64 + 6), M = 5, widths cycling through {1, 3, 4, 8, 12, 13}: strided sources, destinations that are column slices of one
    canary-filled matrix with gaps; every sixth block 16-byte aligned on both sides (float4 path), the others as they fall (scalar path).
    Bit-exact on random 32-bit patterns (NaN payloads); the gaps keep their canary."""
    widths = [[1, 3, 4, 8, 12, 13][k % 6] for k in range(70)]
    srcs, dsts = run_copy_blocks(5, widths, 0, None, 41, align4_every=3)
    v4 = [k for k in range(70) if widths[k] % 4 == 0 and srcs[k].data_ptr() % 16 == 0 and dsts[k].data_ptr() % 16 == 0 and dsts[k].stride(0) % 4 == 0]
    assert any(k < 64 for k in v4) and any(k >= 64 for k in v4) and len(v4) < 30


@pytest.mark.parametrize("variant", ["aligned", "src_off_by_one", "odd_dst_ld"])
def test_copy_blocks_wraps_the_1024_block_grid_and_falls_back_to_scalar(variant):
    """M = 4100, widths [260, 259, 4]: M * 260 / 4 = 266500 float4 items > 1024 * 256.  aligned: blocks 0 and 2 take the float4 path; the first
    source one float into its allocation, or an odd destination leading dimension: the scalar path, the same bits."""
    M, widths = 4100, [260, 259, 4]
    if variant == "aligned":
        srcs, dsts = run_copy_blocks(M, widths, 0, 540, 42, align4_every=1)
        assert all(t.data_ptr() % 16 == 0 for t in (srcs[0], dsts[0], srcs[2], dsts[2])) and dsts[0].stride(0) % 4 == 0 and srcs[0].stride(0) % 4 == 0
    elif variant == "src_off_by_one":
        run_copy_blocks(M, widths, 0, 540, 43, first_src_off_by_one=True, align4_every=1)
    else:
        _, dsts = run_copy_blocks(M, widths, 0, 541, 44, align4_every=1)
        assert dsts[0].stride(0) % 2 == 1


@pytest.mark.parametrize("np_dtype", [np.int64, np.int32])
def test_copy_id_blocks_pieces_into_a_send_buffer(np_dtype):
    """[1, w] pieces into a destination-major send buffer (ext_dist._pack_ids): ids travel as fp32 words, so -1, INT64_MIN and words such as
    0x7FC00001 / 0x7F800001 / 0xFFFFFFFF are NaN patterns in flight and must arrive unchanged; empty pieces are skipped"""
    from dlrm_amd import ops
    rng = np.random.default_rng(51)
    lens = [7, 0, 1, 33, 0, 260, 4, 13]
    pieces = [H.id_block(rng, (n,), np_dtype) for n in lens]
    guard = 5
    out = torch.full((sum(lens) + 2 * guard,), CANARY_I, dtype=to_dev(pieces[0]).dtype, device=dev())
    dsts, o = [], guard
    for n in lens:
        dsts.append(out[o:o + n].view(1, n))
        o += n
    ops.copy_id_blocks([to_dev(p).view(1, p.size) for p in pieces], dsts)
    torch.cuda.synchronize()
    want = torch.from_numpy(np.concatenate([np.full(guard, CANARY_I, dtype=np_dtype)] + pieces + [np.full(guard, CANARY_I, dtype=np_dtype)]))
    assert out.dtype == want.dtype and torch.equal(out.cpu(), want)


@pytest.mark.parametrize("np_dtype", [np.int64, np.int32])
def test_copy_id_blocks_source_major_to_global_batch_order(np_dtype):
    """[N, w] column blocks of a source-major receive buffer into one contiguous [N * w] tensor per block (ext_dist.kjt_input_dist's unpack)"""
    from dlrm_amd import ops
    rng = np.random.default_rng(52)
    N, widths = 4, [5, 0, 1, 64, 13]
    rv_np = H.id_block(rng, (N, sum(widths) + 3), np_dtype)
    rv = to_dev(rv_np)
    guard = 6
    srcs, bufs, outs, o = [], [], [], 0
    for w in widths:
        srcs.append(rv[:, o:o + w])
        b = torch.full((N * w + 2 * guard,), CANARY_I, dtype=rv.dtype, device=dev())
        bufs.append(b)
        outs.append(b[guard:guard + N * w])
        o += w
    ops.copy_id_blocks(srcs, [t.view(N, w) for t, w in zip(outs, widths)])
    torch.cuda.synchronize()
    o = 0
    for w, b in zip(widths, bufs):
        want = np.concatenate([np.full(guard, CANARY_I, dtype=np_dtype), rv_np[:, o:o + w].reshape(-1), np.full(guard, CANARY_I, dtype=np_dtype)])
        assert torch.equal(b.cpu(), torch.from_numpy(want)), w
        o += w


def test_copy_id_blocks_refuses_mixed_dtypes_and_strided_rows():
    from dlrm_amd import ops
    a64 = torch.zeros((3, 8), dtype=torch.int64, device=dev())
    a32 = torch.zeros((3, 8), dtype=torch.int32, device=dev())
    with pytest.raises(RuntimeError):
        ops.copy_id_blocks([a32], [a64])
    with pytest.raises(RuntimeError):
        ops.copy_id_blocks([a64[:, ::2]], [torch.zeros((3, 4), dtype=torch.int64, device=dev())])
    with pytest.raises(RuntimeError):
        ops.copy_id_blocks([a64.float()], [a64.float()])
    assert not a64.any() and not a32.any()


@pytest.mark.parametrize("M,K,Kp", [(1, 1, 4), (7, 13, 16), (33, 479, 480), (5, 16, 16), (2200, 479, 480)])
def test_pad_cols_strided_source_guarded_destination(M, K, Kp):
    """dlrm_pad_cols with a strided source and a destination of leading dimension Kp + 4 (canary columns): columns < K bit-exact on random
    32-bit patterns, pad columns exactly +0.0 (all 32 bits clear); (2200, 479, 480) is 1056000 elements > 4096 * 256: the loop wraps its grid.
    ops.pad_cols (contiguous destination) returns the same matrix."""
    from dlrm_amd import ops
    lib, st = lib_and_stream()
    rng = np.random.default_rng(M + K)
    big = H.random_bits_f32(rng, (M, K + 5))
    src = to_dev(big)[:, 2:2 + K]
    dst = f32_canary((M, Kp + 4))
    assert lib.dlrm_pad_cols(M, K, Kp, ptr(src), src.stride(0), ptr(dst), Kp + 4, st) == 0
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(bits32(got[:, :K]), bits32(big[:, 2:2 + K])) and not bits32(got[:, K:Kp]).any() and canary_intact(dst[:, Kp:])
    plain = ops.pad_cols(src, Kp)
    assert plain.shape == (M, Kp) and np.array_equal(bits32(plain.cpu().numpy()), bits32(got[:, :Kp]))


# ================================================================================================ 5. dense updates
LR = 0.1


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 2048 * 256 * 4 + 5])
def test_sgd_dense_is_one_exact_fma_at_every_alignment(n):
    """ops.sgd_dense: w = fma(-float32(lr), g, w), BIT-EXACT against H.fma32 (one rounding of the exact value; a quarter of the elements
    cancel, so a separate multiply and add would give 0 where the fma gives the product's rounding error).  w and g each 16-byte aligned or
    one float off (all four combinations from n = 5 on; n4 = 0, the scalar loop, whenever either is off); lr by value and from a device
    scalar; the last n wraps the 2048-block grid in both loops.  Guard elements on both sides of w."""
    from dlrm_amd import ops
    rng = np.random.default_rng(n)
    w0, g0 = H.sgd_case(rng, n, LR)
    want = bits32(H.fma32(-np.float32(LR), g0, w0))
    lr_dev = torch.tensor([LR], dtype=torch.float32, device=dev())
    combos = [(0, 0), (1, 0), (0, 1), (1, 1)] if n >= 5 else [(0, 0), (1, 1)]
    for kw, kg in combos:
        for lr in (LR, lr_dev):
            w, wbuf = guarded_f32(w0, kw)
            g, _ = guarded_f32(g0, kg)
            ops.sgd_dense(w, g, lr)
            torch.cuda.synchronize()
            got = bits32(w.cpu().numpy())
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (kw, kg, isinstance(lr, torch.Tensor), bad.size, bad[:4], w0[bad[:4]], g0[bad[:4]])
            assert guards_intact(wbuf, w) and np.array_equal(bits32(g.cpu().numpy()), bits32(g0))


def test_sgd_dense_multi_50_tensors_cross_a_launch_group():
    """ops.sgd_dense_multi on 50 tensors (48 + 2), sizes cycling through {1, 3, 4095, 4096, 4097, 8193} (one chunk of 4096, its neighbours, a
    third chunk of one element), w and g of a tensor aligned or one float off in all four combinations: bit-exact against H.fma32, lr by value
    and from a device scalar, canary guards between the tensors of the one buffer they are carved from"""
    from dlrm_amd import ops
    rng = np.random.default_rng(50)
    sizes = [[1, 3, 4095, 4096, 4097, 8193][k % 6] for k in range(50)]
    starts, o = [], 8
    for k, n in enumerate(sizes):
        o = (o + 3) // 4 * 4
        starts.append((o + (k // 6) % 2, o + (k // 12) % 2))                        # (w start, g start): k // 6 and k // 12 walk the combinations per size
        o += n + 8
    cases = [H.sgd_case(rng, n, LR) for n in sizes]
    lr_dev = torch.tensor([LR], dtype=torch.float32, device=dev())
    for lr in (LR, lr_dev):
        wbuf, gbuf = f32_canary((o + 8,)), f32_canary((o + 8,))
        want = np.full(o + 8, CANARY_F, dtype=np.float32)
        ws, gs = [], []
        for (a, b), n, (w0, g0) in zip(starts, sizes, cases):
            ws.append(wbuf[a:a + n]); gs.append(gbuf[b:b + n])
            ws[-1].copy_(torch.from_numpy(w0)); gs[-1].copy_(torch.from_numpy(g0))
            want[a:a + n] = H.fma32(-np.float32(LR), g0, w0)
        assert {(w.data_ptr() % 16, g.data_ptr() % 16) for w, g in zip(ws, gs)} == {(0, 0), (4, 0), (0, 4), (4, 4)}
        ops.sgd_dense_multi(ws, gs, lr)
        torch.cuda.synchronize()
        got = bits32(wbuf.cpu().numpy())
        bad = np.flatnonzero(got != bits32(want))
        assert bad.size == 0, (isinstance(lr, torch.Tensor), bad.size, bad[:4])


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 3])
def test_adagrad_dense_sum_exact_and_step_within_its_roundings(n, k):
    """ops.adagrad_dense: sum = fma(g, g, sum) BIT-EXACT (H.fma32).  w = fma(-clr, g / (sqrt(s) + eps), w): with q the float64 value of
    g / (sqrt(s) + eps) at the stored fp32 s, |got - ref| <= 8 2^-24 clr |q| + 2^-24 |ref| (H.adagrad_w_bound): sqrt, add and divide round the
    quotient, the FMA rounds the result once.  csrc/Makefile compiles with -O3 and neither -ffast-math nor
    -fno-hip-fp32-correctly-rounded-divide-sqrt, so hipcc's default holds: divide and sqrt are correctly rounded and the doubling of the
    quotient's bound is slack, not needed.  Where g = 0 and sum = 0 (eps > 0) w keeps its bits and sum stays exactly 0.  Aligned and one float
    off a 16-byte boundary; the last n wraps the 4096-block grid; guards around w and sum."""
    from dlrm_amd import ops
    rng = np.random.default_rng(n + k)
    clr, eps = 0.01, 1e-8
    w0, g0 = H.mixed32(rng, n), H.mixed32(rng, n)
    s0 = np.abs(H.mixed32(rng, n))
    s0[rng.random(n) < 0.2] = 0                            # a first step: sum = g^2, sqrt(sum) = |g|
    dead = rng.random(n) < 0.1
    dead[0] = n > 1
    g0[dead], s0[dead] = 0, 0
    s_want = H.fma32(g0, g0, s0)
    ref, bound = H.adagrad_w_bound(w0, g0, s_want, clr, eps)
    clr_dev = torch.tensor([clr], dtype=torch.float32, device=dev())
    for lr in (clr, clr_dev):
        w, wbuf = guarded_f32(w0, k)
        s, sbuf = guarded_f32(s0, k)
        g, _ = guarded_f32(g0, k)
        ops.adagrad_dense(w, s, g, lr, eps)
        torch.cuda.synchronize()
        assert np.array_equal(bits32(s.cpu().numpy()), bits32(s_want))
        got = w.cpu().numpy()
        err = np.abs(got.astype(np.float64) - ref)
        bad = np.flatnonzero(~(err <= bound))
        assert bad.size == 0, (bad.size, bad[:4], got[bad[:4]], ref[bad[:4]], bound[bad[:4]])
        assert np.array_equal(bits32(got[dead]), bits32(w0[dead])) and not bits32(s.cpu().numpy()[dead]).any()
        assert guards_intact(wbuf, w) and guards_intact(sbuf, s)
