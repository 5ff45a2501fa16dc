"""CPU-only: the MLP GEMM dispatch as the library itself reports it (dlrm_linear_*_route: csrc/gemm.hip gemm_route, the host code the calls
run before they launch) against the case table of tests/gemm_route_cases.py.

  * pinning       every row's route is the one written in the table;
  * completeness  every gemm3_kernel / gemm_f32_kernel instantiation in the built library is selected by a row, or listed with a reason;
                  each "unreachable" reason is proved by a sweep of the query that never meets the variant;
  * boundaries    around every workgroup-count threshold of the tile rule the route is a function of the documented inputs and is one the
                  table has a row for — a threshold edit that opens a route no row tests fails here.
"""
import itertools
import re

import pytest

import gemm_route_cases as G
from gemm_route_cases import DGRAD, FWD, WGRAD, Case


def compiled_instantiations():
    from dlrm_amd import _lib
    _lib.load()
    blob = open(_lib.LIB_PATH, "rb").read()
    g3 = set(m.group(0).decode() for m in re.finditer(rb"gemm3_kernelI(?:L[bi]\d+E)+", blob))
    f32 = set(m.group(0).decode() for m in re.finditer(rb"gemm_f32_kernelI(?:L[bi]\d+E)+", blob))
    return g3, f32


def variant(route):
    """a route without the two fields that scale with the shape (splits, kchunk)"""
    return tuple(route[:8]) + tuple(route[10:])


@pytest.mark.parametrize("case", G.CASES, ids=[c.name for c in G.CASES])
def test_route_is_pinned(case):
    assert tuple(G.query(case)) == G.EXPECT[case.name]


def test_table_and_expectations_list_the_same_cases():
    assert set(G.EXPECT) == set(G.BY_NAME)
    for a, b in G.EQUIVALENT:
        ca, cb = G.BY_NAME[a], G.BY_NAME[b]
        assert (ca.entry, ca.M, ca.N, ca.K, ca.act, ca.arith) == (cb.entry, cb.M, cb.N, cb.K, cb.act, cb.arith)
        # two different routes — except on the 64 x 64 tiles, which read no sign bits: there the pair pins "bits given = the fp32 mask"
        assert G.EXPECT[a] != G.EXPECT[b] or G.EXPECT[a][1:3] == (1, 1), (a, b)


def test_every_compiled_instantiation_has_a_case_or_a_reason():
    g3, f32 = compiled_instantiations()
    compiled = g3 | f32
    assert len(g3) >= 1 and len(f32) == 3
    selected = set()
    for c in G.CASES:
        k = G.kernel_name(c.entry, G.query(c))
        if k is not None:
            assert k in compiled, (c.name, k, "the route names a kernel the library does not contain")
            selected.add(k)
    listed = set(G.UNREACHABLE) | set(G.VIA_GEMM_BF16)
    assert not (listed - compiled), ("listed but not compiled", sorted(listed - compiled))
    assert not (listed & selected), ("listed as unreachable / indirect but selected by a case", sorted(listed & selected))
    assert not (set(G.UNREACHABLE) & set(G.VIA_GEMM_BF16))
    uncovered = compiled - selected - listed
    print("gemm instantiations: %d compiled, %d selected by the table, %d unreachable, %d via dlrm_gemm_bf16, %d uncovered"
          % (len(compiled), len(selected), len(G.UNREACHABLE), len(G.VIA_GEMM_BF16), len(uncovered)))
    assert not uncovered, sorted(uncovered)
    for why in G.UNREACHABLE.values():
        assert why.startswith("unreachable in the product build because ")
    for why in G.VIA_GEMM_BF16.values():
        assert why.startswith("reached only through dlrm_gemm_bf16, covered by ")


# shapes of the sweeps: tile edges of all three tile heights, the reduction lengths of both sides of k % 16, N = 1, K <= 16
_ROWS = (1, 16, 70, 256, 304, 1040, 1500, 1990, 4080, 4096, 8100, 16400, 66000)
_COLS = (1, 16, 20, 68, 132, 516, 1020, 2044, 4092)
_ARITH = ("f32", "bf16x6", "bf16")


def _sweep_cases(entry):
    """a grid over shapes and every alignment / option flag the dispatch reads, for one entry point"""
    for M, N, K, arith in itertools.product(_ROWS, _COLS, _COLS, _ARITH):
        if entry == FWD:
            for act, bits, boff, yoff in ((0, 0, 0, 0), (1, 1, 0, 0), (1, 1, 4, 0), (2, 0, 0, 0), (1, 0, 0, 4)):
                yield Case("s", FWD, M, N, K, act=act, arith=arith, mask="bits" if bits else "none",
                           off=(("bias", boff), ("y", yoff)))
            yield Case("s", FWD, M, N, K, arith=arith, bias=False)
        elif entry == DGRAD:
            for mask, act in (("none", 0), ("fp32", 1), ("bits", 1), ("fp32", 2)):
                yield Case("s", DGRAD, M, N, K, act=act, arith=arith, mask=mask)
            yield Case("s", DGRAD, M, N, K, act=1, arith=arith, mask="bits", off=(("xact", 4),))
            yield Case("s", DGRAD, M, N, K, arith=arith, off=(("dx", 4),))
        else:
            for ws, acc, dwoff in ((True, False, 0), (False, False, 0), (True, True, 0), (False, True, 0), (False, False, 4), (True, False, 4)):
                yield Case("s", WGRAD, M, N, K, arith=arith, ws=ws, accumulate=acc, off=(("dw", dwoff),))
            if K > 4:
                yield Case("s", WGRAD, M, N, K, arith=arith, K_store=K - 3)


@pytest.mark.parametrize("entry", [FWD, DGRAD, WGRAD])
def test_unreachable_instantiations_never_appear(entry):
    """the proof behind every "unreachable in the product build" entry: over the whole grid the query never names one of them (and it
    does name every reachable variant of the form, so the grid is not blind)"""
    a, b = G.FORM[entry]
    mine = {k for k in G.UNREACHABLE if k.startswith("gemm3_kernelILb%dELb%dE" % (a, b))}
    assert mine
    seen, n = set(), 0
    for c in _sweep_cases(entry):
        k = G.kernel_name(entry, G.query(c))
        n += 1
        assert k not in mine, (c, k)
        seen.add(k)
    reachable = {G.kernel_name(c.entry, G.query(c)) for c in G.CASES if c.entry == entry} - {None}
    assert reachable <= seen, ("the sweep misses variants the table reaches", sorted(reachable - seen))
    assert n > 5000


def _boundary_shapes():
    """(rows, columns) of an output with one tile fewer, exactly, and one tile more than each workgroup-count threshold of the tile rule
    (128 and 512 workgroups of 128- / 256-row tiles, 192 of 64-row tiles), over 1, 8 and 16 column tiles"""
    out = set()
    for cols, ct in ((68, 1), (1020, 8), (2044, 16)):
        for thr, h in itertools.product((128, 192, 512), (64, 128, 256)):
            for r in (thr // ct - 1, thr // ct, thr // ct + 1):
                if r >= 1:
                    out.update({(r * h - 3, cols), (r * h, cols), (r * h + 1, cols)})
    return sorted(out)


def _wgrad_boundary_shapes():
    """(M, N, K) of weight gradients on either side of each threshold WITH the k-slices counted: the rule compares
    tiles x splits (wg128 < 128, wg64 < 192, wg256 >= 512), and splits is wgrad_plan's answer for the batch.  For each output shape
    the batch is swept in steps of 16 rows, the library is asked for its split count, and the batches whose workgroup count is the
    largest below and the smallest at or above each threshold are kept (with their neighbours 16 rows away)."""
    out = set()
    for n, k in ((68, 68), (132, 132), (260, 516), (516, 516), (1500, 132), (4092, 260), (1020, 1020), (2040, 1020), (68, 2044), (1020, 2040)):
        splits = {}
        for m in range(16, 16400 + 1, 16):
            r = G.query(Case("p", WGRAD, m, n, k))
            if r.path in (0, 1):
                splits[m] = r.splits
        for thr, h in ((128, 128), (192, 64), (512, 256)):
            wg = {m: -(-n // h) * -(-k // 128) * s for m, s in splits.items()}
            below = [m for m in wg if wg[m] < thr]
            above = [m for m in wg if wg[m] >= thr]
            picks = []
            if below:
                top = max(wg[m] for m in below)
                picks += [min(m for m in below if wg[m] == top), max(m for m in below if wg[m] == top)]
            if above:
                low = min(wg[m] for m in above)
                picks += [min(m for m in above if wg[m] == low), max(m for m in above if wg[m] == low)]
            for m in picks:
                out.update((mm, n, k) for mm in (m - 16, m, m + 16) if mm in splits)
    return sorted(out)


@pytest.mark.parametrize("entry", [FWD, DGRAD, WGRAD])
def test_routes_around_the_thresholds_are_in_the_table(entry):
    table = {(c.entry, variant(G.EXPECT[c.name])) for c in G.CASES}
    missing = {}
    groups = []
    if entry == WGRAD:
        shapes = _wgrad_boundary_shapes()
        assert len(shapes) >= 20
        groups = [[Case("b", WGRAD, m, n, k, arith=ar, ws=ws, accumulate=acc)
                   for ar in _ARITH for ws, acc in ((True, False), (False, False), (True, True), (False, True))] for m, n, k in shapes]
    for rows, cols in _boundary_shapes():
        if entry == FWD:
            cs = [Case("b", FWD, rows, cols, k, act=act, arith=ar, mask=m, off=off)
                  for k in (16, 80) for ar in _ARITH for act, m, off in ((0, "none", ()), (1, "bits", ()), (1, "bits", (("bias", 4),)), (2, "none", ()))]
        elif entry == DGRAD:
            cs = [Case("b", DGRAD, rows, n, cols, act=act, arith=ar, mask=m)
                  for n in (16, 80) for ar in _ARITH for act, m in ((0, "none"), (1, "fp32"), (1, "bits"))]
        else:           # the weight gradient's counts include the k-slices: its shapes come from _wgrad_boundary_shapes above
            continue
        groups.append(cs)
    for cs in groups:
        for c in cs:
            r1 = G.query(c)
            moved = {op: a + 0x1000 for op, a in G.fake_addresses(c).items()}       # other addresses, same alignment
            assert r1 == G.query(c) == G.query(c, moved), c
            if (entry, variant(r1)) not in table:
                missing.setdefault(variant(r1), c)
    assert not missing, "routes near a threshold that no case of tests/gemm_route_cases.py tests: %r" % (missing,)


def test_route_queries_refuse_what_the_calls_refuse():
    """the query runs the call's own argument checks: same error codes, nothing written"""
    from dlrm_amd import ops
    with pytest.raises(RuntimeError, match="DLRM_E_ARG"):
        ops.linear_fwd_route(0, 4, 4, 16, 4, 32, 4, None, 0, 64, 4)
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.linear_fwd_route(8, 4, 4, 16, 4, 32, 4, None, 0, 64, 4, relu_bits=128)            # sign bits without ReLU
    with pytest.raises(RuntimeError, match="DLRM_E_ARG"):
        ops.linear_bwd_weight_route(64, 8, 8, 5, 16, 8, 32, 8, 64, 8)                         # K_store < K without the workspace
