"""dlrm_stage_inputs (csrc/stage.hip) against torch copies, byte for byte.  Every source and destination lives inside one byte arena at
a chosen offset from a 16-byte boundary, each destination is followed by a guard word, and the whole destination arena is compared with
what torch's own copies make of it: a byte written outside a segment, or not written inside one, shows."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 0x5A


def _stage(segs, stream=None):
    from dlrm_amd import _lib
    n = len(segs)
    dst = (C.c_void_p * max(n, 1))(*[d for d, _, _ in segs])
    src = (C.c_void_p * max(n, 1))(*[s for _, s, _ in segs])
    nb = (C.c_int64 * max(n, 1))(*[b for _, _, b in segs])
    rc = _lib.load().dlrm_stage_inputs(n, dst, src, nb, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc


def _run(cases):
    """cases: (nbytes, source misalignment, destination misalignment); returns nothing, asserts equality with torch's copies"""
    dev = torch.device("cuda:0")
    slot = lambda nb: ((nb + 16 + 15) // 16) * 16 + 16          # noqa: E731  (payload + guard, then the next 16-byte boundary + room to shift)
    total = sum(slot(nb) for nb, _, _ in cases) + 64
    g = torch.Generator().manual_seed(len(cases))
    src_arena = torch.randint(0, 256, (total,), dtype=torch.uint8, generator=g).to(dev)
    dst_arena = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
    assert src_arena.data_ptr() % 16 == 0 and dst_arena.data_ptr() % 16 == 0
    want = dst_arena.clone()
    segs, at = [], 0
    for nb, ms, md in cases:
        so, do = at + ms, at + md
        segs.append((dst_arena.data_ptr() + do, src_arena.data_ptr() + so, nb))
        want[do:do + nb] = src_arena[so:so + nb]               # torch's copy of the same bytes
        at += slot(nb)
    assert _stage(segs) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst_arena, want)                         # payloads AND every guard byte


LENGTHS = (0, 4, 8, 12, 16, 20, 4100)


def test_one_segment_every_length():
    for nb in LENGTHS:
        _run([(nb, 0, 0)])


@pytest.mark.parametrize("ms", (0, 4, 8))
@pytest.mark.parametrize("md", (0, 4, 8))
def test_misaligned_sources_and_destinations(ms, md):
    """(0, 0) (4, 4) (8, 8): 16-byte bodies with 4-byte words in front and behind; a difference of 8: 8-byte bodies; of 4: words"""
    _run([(nb, ms, md) for nb in LENGTHS])


def test_sixty_five_segments_take_two_launches():
    cases = [(LENGTHS[k % len(LENGTHS)], 4 * (k % 3), 4 * ((k // 3) % 3)) for k in range(65)]
    cases[64] = (20, 4, 8)                                      # (the one segment of the second launch copies something)
    _run(cases)


@pytest.mark.parametrize("dtype", (torch.int32, torch.int64, torch.float32))
def test_payload_types_against_tensor_copies(dtype):
    """a request as GraphedForward stages it: tensors of n elements into the heads of longer static tensors"""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    ns = (1, 5, 513)
    if dtype == torch.float32:
        srcs = [torch.randn(n, generator=g).to(dev) for n in ns]
    else:
        srcs = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int64, generator=g).to(dtype).to(dev) for n in ns]
    dsts = [torch.full((n + 3,), 77, dtype=dtype, device=dev) for n in ns]
    want = [d.clone() for d in dsts]
    for w, s in zip(want, srcs):
        w[:s.numel()].copy_(s)
    assert _stage([(d.data_ptr(), s.data_ptr(), s.numel() * s.element_size()) for d, s in zip(dsts, srcs)]) == 0
    torch.cuda.synchronize()
    for d, w in zip(dsts, want):
        assert torch.equal(d.view(torch.uint8), w.view(torch.uint8))


def test_source_equal_to_destination_is_skipped_and_bad_arguments_are_refused():
    from dlrm_amd import _lib
    dev = torch.device("cuda:0")
    a = torch.arange(64, dtype=torch.int32, device=dev)
    b = torch.zeros(64, dtype=torch.int32, device=dev)
    keep = a.clone()
    assert _stage([(a.data_ptr(), a.data_ptr(), 256), (b.data_ptr(), a.data_ptr(), 128)]) == 0
    assert _stage([(a.data_ptr(), a.data_ptr(), 256)]) == 0     # nothing to copy at all: no launch
    assert _stage([]) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, keep) and torch.equal(b[:32], keep[:32]) and int(b[32:].abs().sum()) == 0
    # 2-byte alignment or length: refused before anything is launched
    assert _stage([(b.data_ptr() + 2, a.data_ptr(), 8)]) == -2
    assert _stage([(b.data_ptr(), a.data_ptr(), 6)]) == -2
    assert _stage([(b.data_ptr(), 0, 8)]) == -1 and _stage([(b.data_ptr(), a.data_ptr(), -4)]) == -1
    with pytest.raises(RuntimeError, match="DLRM_E_ALIGN"):
        _lib.check(-2, "dlrm_stage_inputs")
