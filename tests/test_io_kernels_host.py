"""Host restatements and case builders for the metrics, input, copy and dense-update kernels (csrc/metrics.hip, csrc/datagen.hip,
csrc/multihot.hip, csrc/loss_opt.hip, csrc/adagrad.hip), the part that needs no GPU.

tests/test_gpu_io_kernels.py imports this file as `H`.  The references of those tests are the oracle functions of oracle/oracle.py (pinned to
the reference and to scikit-learn by tests/test_oracle_golden.py); what this file adds, and proves on the CPU, is

  * the score / target families of the metrics tests, an independent restatement of the metrics over the DISTINCT thresholds in exact
    integer / rational arithmetic, and the check of `O.binary_metrics` against it and against scikit-learn on those families;
  * the synthetic raw Criteo records (dense counts 0, -1, -2, 2^31-1; ids 0, -1, INT32_MIN, INT32_MAX, multiples of the range);
  * a row-range restatement of the uniform multi-hot lookup table, pinned to `O.philox_multihot_table`;
  * random 32-bit patterns (NaN payloads included) and the id values whose words are NaN patterns, for the block copies;
  * `fma32`: one fp32 fused multiply-add, exactly (product in float64, TwoSum residual decides the fp32 midpoints), proven against
    fractions.Fraction; the error bound of the dense Adagrad step.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
from oracle import oracle as O  # noqa: E402

U24 = 2.0 ** -24                       # half an fp32 ulp, relative
U53 = 2.0 ** -53                       # half an fp64 ulp, relative
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
INT64_MIN = -2 ** 63


# ------------------------------------------------------------------------------------------------ metrics: inputs
METRIC_SIZES = [1, 2, 255, 256, 257, 262144 + 257]      # the last wraps the grid of 1024 blocks x 256 threads
ROUND_EDGES = np.array([0.5, 1.5, 2.5, -0.5, 0.49999997, 0.50000006, 1.0, 2.0, -3.0], dtype=np.float32)
METRIC_FAMILIES = ["logits", "k1", "k2", "k3", "k17", "edges", "distinct"]


def metric_targets(rng, n, frac=0.3):
    return (rng.random(n) < frac).astype(np.float32)


def metric_case(family, n, seed=0):
    """(scores, targets) float32 [n] of one family:
    logits   N(0, 2) rounded to one decimal (long tie groups, negative values), every 5th element -0.0 and the next one +0.0
    k<K>     K distinct values j / K: tie groups far longer than a block, across every block boundary and the grid wrap
    edges    the np.round edges, every (value, target) pair present from n >= 18 on
    distinct a permutation of arange(n) / n: no ties at all"""
    rng = np.random.default_rng(1000 * seed + n % 9973 + 17 * METRIC_FAMILIES.index(family))
    t = metric_targets(rng, n)
    if family == "logits":
        s = np.round(rng.standard_normal(n) * 2.0, 1).astype(np.float32)
        s[0::5] = np.float32(-0.0)
        s[1::5] = np.float32(0.0)
    elif family.startswith("k"):
        k = int(family[1:])
        s = (rng.integers(0, k, size=n) / np.float64(k)).astype(np.float32)
    elif family == "edges":
        i = np.arange(n)
        s = ROUND_EDGES[i % ROUND_EDGES.size].copy()
        t = ((i // ROUND_EDGES.size) % 2).astype(np.float32)
        p = rng.permutation(n)
        s, t = s[p], t[p]
    elif family == "distinct":
        s = (rng.permutation(n) / np.float64(n)).astype(np.float32)
        assert np.unique(s).size == n
    else:
        raise ValueError(family)
    return s, t


def distinct_scores(s):
    """number of distinct thresholds (-0.0 and +0.0 are one)"""
    return int(np.unique(np.asarray(s, dtype=np.float32) + np.float32(0.0)).size)


def ap_bound(G, ref):
    """|got - ref| <= 2 (G + 2) 2^-53 ref: a sum of G non-negative fp64 terms, each one rounded division times one rounded product, accumulated in
    any order ((G - 1) roundings at most on any term's path) and divided once, on BOTH sides (hence the factor 2)"""
    return 2.0 * (G + 2) * U53 * abs(ref)


COUNTERS = ("n", "positives", "tp", "fp", "fn", "tn", "round_matches")


def metrics_restated(s, t):
    """The metrics from the per-threshold class counts, O(G) after one np.unique: counters by Python's round() (half to even on the exact value),
    roc_auc = (sum of d_fp (tp + tp_prev)) / (2 P N) in integers with ONE correctly rounded division, ap as an exact Fraction rounded once."""
    s = np.asarray(s, dtype=np.float32).reshape(-1)
    t = np.asarray(t, dtype=np.float32).reshape(-1)
    y = t > 0.5
    r = np.array([round(float(v)) for v in s], dtype=np.float64)
    pred = r > 0.5
    out = dict(n=int(s.size), positives=int(y.sum()), tp=int((pred & y).sum()), fp=int((pred & ~y).sum()), fn=int((~pred & y).sum()),
               tn=int((~pred & ~y).sum()), round_matches=int((r == t.astype(np.float64)).sum()))
    vals, inv = np.unique(s.astype(np.float64) + 0.0, return_inverse=True)      # ascending; -0.0 + 0.0 == +0.0
    pos = np.bincount(inv, weights=y.astype(np.float64), minlength=vals.size).astype(np.int64)[::-1]
    cnt = np.bincount(inv, minlength=vals.size).astype(np.int64)[::-1]
    P, n = int(pos.sum()), int(cnt.sum())
    N = n - P
    tp = seen = 0
    auc2, ap = 0, Fraction(0)
    for p_g, c_g in zip(pos.tolist(), cnt.tolist()):
        tp_prev = tp
        tp += p_g
        seen += c_g
        auc2 += (c_g - p_g) * (tp + tp_prev)
        if p_g:
            ap += Fraction(p_g * tp, seen)
    out["roc_auc"] = auc2 / (2 * P * N) if P and N else float("nan")     # int / int: correctly rounded
    out["ap"] = float(ap / P) if P else float("nan")
    out["G"] = int(vals.size)
    return out


# ------------------------------------------------------------------------------------------------ Criteo raw records
CRITEO_B = [1, 63, 64, 65, 300]
CRITEO_RANGES = [-1, 0, 1, 1000, 40000000]


def criteo_raw(B, max_ind_range, seed=0):
    """int32 [B, 40] raw records: label 0/1 | 13 dense counts | 26 categorical ids, with the edge values of both at fixed positions"""
    rng = np.random.default_rng(seed + 31 * B)
    raw = np.empty((B, 40), dtype=np.int64)
    raw[:, 0] = rng.integers(0, 2, size=B)
    raw[:, 1:14] = rng.integers(0, 5000, size=(B, 13))
    raw[:, 14:] = rng.integers(INT32_MIN, INT32_MAX + 1, size=(B, 26))
    dense_edges = [0, -1, -2, INT32_MAX]
    m = max(int(max_ind_range), 1)
    id_edges = [0, -1, INT32_MIN, INT32_MAX, m, -m, (INT32_MAX // m) * m, -((2 ** 31) // m) * m, 3 * m if 3 * m <= INT32_MAX else m]
    for b in range(B):                                   # every record carries some edges, rotating through the columns
        for k, v in enumerate(dense_edges):
            raw[b, 1 + (b + 3 * k) % 13] = v
        for k, v in enumerate(id_edges):
            raw[b, 14 + (b + 5 * k) % 26] = v
    assert raw.min() >= INT32_MIN and raw.max() <= INT32_MAX
    return raw.astype(np.int32)


def ulp_distance32(a, b):
    """distance in representable fp32 values between finite a and b of equal sign (or zero)"""
    ia = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, INT32_MIN - ia, ia)            # sign-magnitude -> a monotone integer line
    ib = np.where(ib < 0, INT32_MIN - ib, ib)
    return np.abs(ia - ib)


def criteo_log_ref(raw):
    """log(float32(count) + 1) with the logarithm taken in float64 and rounded once: the correctly rounded fp32 value"""
    x = raw[:, 1:14].astype(np.float32) + np.float32(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(x.astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ multi-hot table rows
_M32 = np.uint64(0xFFFFFFFF)


def multihot_uniform_rows(table_id, rows, hot, seed, r0, r1):
    """rows r0 .. r1-1 of dlrm_multihot_gen_table(dist = uniform): column 0 the row number, element (r, c >= 1) = (word 0 of Philox block
    (r lo, r hi, c, 0xC0000000 | table_id) * rows) >> 32"""
    r = np.arange(r0, r1, dtype=np.uint64)
    out = np.empty((r.size, hot), dtype=np.int32)
    out[:, 0] = np.arange(r0, r1)
    for c in range(1, hot):
        w = O.philox4x32(r & _M32, r >> np.uint64(32), c, 0xC0000000 | table_id, seed)
        out[:, c] = ((w[0] * np.uint64(rows)) >> np.uint64(32)).astype(np.int32)
    return out


# ------------------------------------------------------------------------------------------------ copies
def random_bits_f32(rng, shape):
    """uniform random 32-bit patterns viewed as fp32: every NaN payload, infinity and subnormal class turns up"""
    return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)


NAN_WORDS = [0x7FC00001, 0x7F800001, 0xFFFFFFFF]        # quiet NaN with payload, signalling NaN, all ones


def special_ids(dtype):
    """ids whose 32-bit words are NaN bit patterns when looked at as fp32, as signed values of `dtype` (np.int32 / np.int64)"""
    if np.dtype(dtype) == np.int32:
        v = [-1, INT32_MIN, INT32_MAX, 0, 1] + [w - 2 ** 32 if w >= 2 ** 31 else w for w in NAN_WORDS]
        return np.array(v, dtype=np.int32)
    v = [-1, INT64_MIN, 2 ** 63 - 1, 0, 1, 39884405]
    for w in NAN_WORDS:
        v += [w, w << 32, (w << 32) | 5, (w << 32) | w]
    return np.array([x - 2 ** 64 if x >= 2 ** 63 else x for x in v], dtype=np.int64)


def id_block(rng, shape, dtype, rows=40000000):
    """ordinary row ids with the special values scattered over a third of the positions"""
    a = rng.integers(0, rows, size=shape).astype(dtype)
    sp = special_ids(dtype)
    hit = rng.random(shape) < 0.34
    a[hit] = sp[rng.integers(0, sp.size, size=int(hit.sum()))]
    flat = a.reshape(-1)
    flat[:min(flat.size, sp.size)] = sp[:flat.size]      # every special value at least once where the block is large enough
    return a


# ------------------------------------------------------------------------------------------------ one exact fp32 FMA
def fma32(a, b, c):
    """round_to_nearest_even_fp32(a * b + c) for fp32 arrays, ONE rounding of the exact value (finite results in the normal fp32 range).
    p = a * b is exact in float64 (48-bit product); s = fl64(p + c) with its exact TwoSum residual e (s + e == p + c).  float32(s) is the answer
    unless s lies exactly on the midpoint of two neighbouring fp32 values while e != 0: the exact value is then off the midpoint on the side of
    e, and the neighbour on that side is the answer.  (If s is not a midpoint, s and s + e lie on the same side of every midpoint, because the
    midpoints are float64 values and s = fl64(s + e).)"""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)                      # TwoSum (Knuth): exact
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    inf = np.float32(np.inf)
    up, dn = np.nextafter(r, inf), np.nextafter(r, -inf)
    mid_up = (s > r64) & (s == 0.5 * (r64 + up.astype(np.float64)))      # s halfway between r and the next value above: RNE chose r
    mid_dn = (s < r64) & (s == 0.5 * (r64 + dn.astype(np.float64)))      # s halfway between the next value below and r: RNE chose r
    return np.where(mid_up & (e > 0), up, np.where(mid_dn & (e < 0), dn, r))


def _round_fraction_f32(x):
    """the fp32 value nearest the Fraction x, ties to the even significand (normal range)"""
    r = np.float32(float(x))
    cands = sorted({float(np.nextafter(r, np.float32(-np.inf))), float(r), float(np.nextafter(r, np.float32(np.inf)))})
    best = min(cands, key=lambda v: (abs(Fraction(v) - x), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def midpoint_triples():
    """(a, b, c) whose exact a * b + c is 2^-70 (relative) off an fp32 midpoint: float64 rounds the sum ONTO the midpoint"""
    one_p, one_m = np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -23)        # (1 + u)(1 - u) = 1 - 2^-46
    out = []
    for scale in (1.0, 2.0 ** 10, 2.0 ** -7, 3.0 * 2.0 ** 5):
        lead = 2.0 ** np.floor(np.log2(scale))
        half = np.float32(lead * 2.0 ** -24)             # half an ulp of c
        for c in (scale, scale * (1 + 2.0 ** -23), scale * (1 + 2.0 ** -22), -scale, -scale * (1 + 2.0 ** -23)):
            for sign in (1.0, -1.0):
                out.append((np.float32(sign) * one_p * half, one_m, np.float32(c)))
                out.append((np.float32(sign) * half, np.float32(1.0), np.float32(c)))            # exactly ON the midpoint: ties to even
    return out


def mixed32(rng, n):
    """fp32 values over six decades, both signs"""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, size=n)).astype(np.float32)


def sgd_case(rng, n, lr):
    """(w, g) with a quarter of the elements cancelling: w = fl(lr * g), so that the fused w - lr g is the product's rounding error and an
    unfused multiply-add gives exactly 0"""
    w, g = mixed32(rng, n), mixed32(rng, n)
    cancel = rng.random(n) < 0.25
    cancel[0] = True
    w[cancel] = np.float32(lr) * g[cancel]
    return w, g


def adagrad_w_bound(w_ref, g, s, clr, eps):
    """|got - ref| <= 8 2^-24 clr |q| + 2^-24 |ref|, q = g / (sqrt(s) + eps) in float64: sqrt, add and divide round the quotient (four roundings
    with the rounded s included, doubled), the final FMA rounds the result once.  Returns (w_ref float64, bound)."""
    g64, s64 = np.asarray(g, dtype=np.float64), np.asarray(s, dtype=np.float64)
    q = g64 / (np.sqrt(s64) + float(np.float32(eps)))
    ref = np.asarray(w_ref, dtype=np.float64) - float(np.float32(clr)) * q
    return ref, 8 * U24 * float(np.float32(clr)) * np.abs(q) + U24 * np.abs(ref)


# ------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("n", [257, 5000])
@pytest.mark.parametrize("family", ["logits", "k1", "k2", "k3", "k17", "edges"])
def test_oracle_metrics_equal_the_per_threshold_restatement(family, n):
    """O.binary_metrics against metrics_restated: counters exact; roc_auc bit-equal (both sides hold the exact numerator: every trapezoid term
    is a multiple of 0.5 below P N < 2^53, and divide once); ap within (G + 2) 2^-53 of the exactly rounded value.  Also bit-stable under a
    permutation of the pairs, and the same with all targets 1 / all 0."""
    s, t = metric_case(family, n)
    for tt in (t, np.ones_like(t), np.zeros_like(t)):
        o, r = O.binary_metrics(s, tt), metrics_restated(s, tt)
        for k in COUNTERS:
            assert o[k] == r[k], (k, o[k], r[k])
        assert r["G"] == distinct_scores(s)
        if np.isnan(r["roc_auc"]):
            assert np.isnan(o["roc_auc"])
        else:
            assert o["roc_auc"] == r["roc_auc"]
        if np.isnan(r["ap"]):
            assert np.isnan(o["ap"])
        else:
            assert abs(o["ap"] - r["ap"]) <= 0.5 * ap_bound(r["G"], r["ap"]), (o["ap"], r["ap"])
        p = np.random.default_rng(5).permutation(n)
        o2 = O.binary_metrics(s[p], tt[p])
        assert all(o2[k] == o[k] or (np.isnan(o2[k]) and np.isnan(o[k])) for k in COUNTERS + ("roc_auc",))
    assert O.binary_metrics(s, np.ones_like(t))["ap"] == 1.0


@pytest.mark.parametrize("n", [257, 5000])
@pytest.mark.parametrize("family", ["logits", "k1", "k2", "k3", "k17", "edges"])
def test_oracle_metrics_equal_scikit_learn(family, n):
    sk = pytest.importorskip("sklearn.metrics")
    s, t = metric_case(family, n)
    o = O.binary_metrics(s, t)
    assert abs(o["roc_auc"] - sk.roc_auc_score(t, s)) <= ap_bound(distinct_scores(s), 1.0)      # scikit-learn sums G rounded fractions
    assert abs(o["ap"] - sk.average_precision_score(t, s)) <= ap_bound(distinct_scores(s), o["ap"])
    pred = np.round(s) > 0.5
    assert o["tp"] + o["tn"] == int(sk.accuracy_score(t > 0.5, pred, normalize=False))


def test_metric_families_hold_what_they_promise():
    s, t = metric_case("logits", 257)
    assert np.signbit(s[0]) and s[0] == 0 and not np.signbit(s[1]) and s[1] == 0 and s.min() < 0 and distinct_scores(s) < 200
    for k in (1, 2, 3, 17):
        assert distinct_scores(metric_case("k%d" % k, 5000)[0]) == k
    s, t = metric_case("edges", 257)
    assert {(float(a), float(b)) for a, b in zip(s, t)} == {(float(a), b) for a in ROUND_EDGES for b in (0.0, 1.0)}
    m = metrics_restated(ROUND_EDGES, np.ones(ROUND_EDGES.size, dtype=np.float32))
    # np.round: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0, 0.50000006 -> 1; a prediction >= 1.5 rounds to 2: positive, never equal to a target
    assert m["tp"] == 5 and m["round_matches"] == 2
    assert metrics_restated(ROUND_EDGES, np.zeros(ROUND_EDGES.size, dtype=np.float32))["round_matches"] == 3     # 0.5, -0.5, 0.49999997
    assert distinct_scores(metric_case("distinct", 262401)[0]) == 262401


def test_criteo_raw_records_hold_every_edge():
    for B in CRITEO_B:
        for m in CRITEO_RANGES:
            raw = criteo_raw(B, m)
            assert raw.shape == (B, 40) and raw.dtype == np.int32 and set(np.unique(raw[:, 0])) <= {0, 1}
            with np.errstate(divide="ignore", invalid="ignore"):             # counts -1 and -2: log 0 and log of a negative, on purpose
                X, lS_o, lS_i, T = O.criteo_bin_transform(raw, m)
            assert np.array_equal(np.isneginf(X), raw[:, 1:14] == -1) and np.array_equal(np.isnan(X), raw[:, 1:14] < -1)
            ref = criteo_log_ref(raw)
            fin = np.isfinite(X)
            assert np.array_equal(np.isfinite(ref), fin) and int(ulp_distance32(X[fin], ref[fin]).max()) <= 1
            ids = raw[:, 14:]
            assert {0, -1, INT32_MIN, INT32_MAX} <= set(ids.reshape(-1).tolist())
            if m > 0:
                assert lS_i.min() >= 0 and lS_i.max() < m and (ids.astype(np.int64) % m == 0).sum() >= B
            else:
                assert np.array_equal(lS_i, ids.T.astype(np.int64)) and lS_i.min() == INT32_MIN
    assert list(ulp_distance32(np.float32([1.0, -1.0, 0.0]), np.float32([1.0000001, -1.0000001, -0.0]))) == [1, 1, 0]


def test_generator_refuses_int32_ids_for_more_than_2_to_31_rows_before_any_gpu_work():
    """the constructor's refusal needs no device: 2^31 rows (largest id 2^31 - 1) is the last size int32 ids address"""
    import torch
    from dlrm_amd.datagen import UniformBatchGenerator
    with pytest.raises(RuntimeError, match="int32"):
        UniformBatchGenerator(4, [10, 2 ** 31 + 1], 2, True, device="cuda:0", index_dtype=torch.int32)
    assert UniformBatchGenerator(4, [10, 2 ** 31], 2, True, device="cuda:0", index_dtype=torch.int32).rows[1] == 2 ** 31
    assert UniformBatchGenerator(4, [10, 2 ** 31 + 1], 2, True, device="cuda:0", index_dtype=torch.int64).rows[1] == 2 ** 31 + 1


def test_multihot_row_range_restatement_equals_the_oracle_table():
    for t, rows, hot, seed in ((0, 1000, 10, 7), (3, 1000, 1, 7), (5, 1000, 4, 99)):
        whole = O.philox_multihot_table(t, rows, hot, 0, seed)
        assert np.array_equal(multihot_uniform_rows(t, rows, hot, seed, 0, rows), whole)
        assert np.array_equal(multihot_uniform_rows(t, rows, hot, seed, 333, 612), whole[333:612])


def test_special_ids_are_nan_words():
    for dt in (np.int32, np.int64):
        sp = special_ids(dt)
        words = sp.view(np.uint32)
        assert all(w in words for w in NAN_WORDS) and -1 in sp and np.iinfo(dt).min in sp
        assert np.isnan(words.view(np.float32)).sum() >= 4
        blk = id_block(np.random.default_rng(0), (6, 31), dt)
        assert blk.dtype == dt and set(sp.tolist()) <= set(blk.reshape(-1).tolist())
    b = random_bits_f32(np.random.default_rng(1), (4000,))
    assert np.isnan(b).any() and b.dtype == np.float32


def test_fma32_is_one_rounding_of_the_exact_value():
    """against fractions.Fraction on 10^4 random triples (a quarter of them cancelling: c = -fl(a b)) and on the constructed midpoint triples,
    where rounding the float64 sum instead gives the wrong neighbour"""
    rng = np.random.default_rng(11)
    n = 10000
    a, b, c = mixed32(rng, n), mixed32(rng, n), mixed32(rng, n)
    cancel = rng.random(n) < 0.25
    c[cancel] = -(a[cancel] * b[cancel])
    near = rng.random(n) < 0.25                          # c of the product's magnitude: the sum's low bits matter
    c[near & ~cancel] = (a * b * rng.uniform(-2, 2, size=n).astype(np.float32))[near & ~cancel]
    got = fma32(a, b, c)
    for i in range(n):
        want = _round_fraction_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)
    assert np.any(got[cancel] != 0)                      # the cancelling triples return the product's rounding error
    tri = midpoint_triples()
    ta, tb, tc = (np.array([x[k] for x in tri], dtype=np.float32) for k in range(3))
    got = fma32(ta, tb, tc)
    naive = (ta.astype(np.float64) * tb.astype(np.float64) + tc.astype(np.float64)).astype(np.float32)
    for i in range(len(tri)):
        want = _round_fraction_f32(Fraction(float(ta[i])) * Fraction(float(tb[i])) + Fraction(float(tc[i])))
        assert got[i] == want, (i, tri[i], got[i], want)
    assert np.any(naive != got)                          # the midpoint cases do tell the two apart
    assert fma32(np.float32(2), np.float32(3), np.float32(1)) == np.float32(7)


def test_sgd_case_cancels_and_adagrad_bound_is_tight_enough_to_matter():
    rng = np.random.default_rng(12)
    w, g = sgd_case(rng, 1000, 0.1)
    fused = fma32(-np.float32(0.1), g, w)
    unfused = (w + (-np.float32(0.1)) * g).astype(np.float32)
    assert np.any(fused != unfused) and np.any((unfused == 0) & (fused != 0))
    s = np.abs(mixed32(rng, 1000)) + np.float32(1e-3)
    ref, bound = adagrad_w_bound(w, g, s, 0.01, 1e-8)
    step = np.abs(ref - w.astype(np.float64))
    assert np.all(bound <= 1e-6 * step + U24 * np.abs(ref))          # far inside the rtol 1e-6 of the first test of this kernel
