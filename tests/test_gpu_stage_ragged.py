"""dlrm_stage_ragged (csrc/stage.hip: stage_ragged_kernel) against torch, byte for byte.  Every destination — the dense buffer, each table's
static ids and static offsets — lives inside ONE byte arena at a chosen 4-byte phase from a 16-byte boundary, with guard bytes on both
sides; the expected arena is made with torch on the host (ids_static[shift:] = ids, offsets = shift + clamp(off, 0, nnz) for b < n and cap
behind) and the WHOLE arena is compared after each call: a byte written outside a buffer, in front of the shifted ids, or not written
inside the offsets, shows."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, OLD = 0x5A, 0x33         # guard bytes around every buffer; what the buffers hold before the call
DT = {4: torch.int32, 8: torch.int64}


class Arena:
    """a byte arena built on the host: take(nbytes, phase) -> the offset of nbytes whose address is `phase` modulo 16, >= 16 guard bytes
    in front and behind"""

    def __init__(self, fill):
        self.fill, self.at, self.parts = fill, 0, []

    def take(self, nbytes, phase=0, data=None, fill=None):
        o = ((self.at + 16 + 15) // 16) * 16 + phase
        self.at = o + nbytes + 16
        self.parts.append((o, nbytes, data, fill))
        return o

    def build(self):
        t = torch.full((self.at + 32,), self.fill, dtype=torch.uint8)
        for o, nb, data, fill in self.parts:
            if data is not None:
                t[o:o + nb] = data.contiguous().view(torch.uint8).reshape(-1)
            elif fill is not None:
                t[o:o + nb] = fill
        return t


def _stage(x, ids, offs, n, bucket, elem):
    """x = (dst, src, bytes); ids / offs = lists of (dst, src, nnz, cap), pointers as ints (0: null)"""
    from dlrm_amd import _lib

    def arrays(segs):
        m = max(len(segs), 1)
        return ((C.c_void_p * m)(*[s[0] or None for s in segs]), (C.c_void_p * m)(*[s[1] or None for s in segs]),
                (C.c_int64 * m)(*[s[2] for s in segs]), (C.c_int64 * m)(*[s[3] for s in segs]))
    return _lib.load().dlrm_stage_ragged(C.c_void_p(x[0] or None), C.c_void_p(x[1] or None), x[2], len(ids), *arrays(ids), len(offs), *arrays(offs),
                                         n, bucket, elem, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def want_offsets(off, n, bucket, nnz, cap, dtype):
    """the static offsets as the issue defines them, with torch"""
    out = torch.full((bucket,), cap, dtype=torch.int64)
    out[:n] = (cap - nnz) + off[:n].to(torch.int64).clamp(0, nnz)
    return out.to(dtype)


def _run(elem, bucket, n, tables, m_den=4, seed=0, share_offsets=False, x_phase=(0, 0)):
    """tables: dicts with cap, nnz and optionally off (n request offsets, any values), ids_phase / off_phase = (source, destination) phases.
    share_offsets: ONE offsets segment (table 0's) for all tables.  Stages once and compares the whole destination arena."""
    dev = torch.device("cuda:0")
    dt = DT[elem]
    g = torch.Generator().manual_seed(seed)
    src, dst = Arena(0), Arena(GUARD)
    X = torch.rand((n, m_den), generator=g)
    xs, xd = src.take(n * m_den * 4, x_phase[0], data=X), dst.take(bucket * m_den * 4, x_phase[1], fill=OLD)
    lay = []
    for k, t in enumerate(tables):
        cap, nnz = t["cap"], t["nnz"]
        ids = torch.randint(0, 2 ** 31 - 1, (nnz,), generator=g, dtype=torch.int64).to(dt)
        off = t.get("off")
        if off is None:
            off = torch.sort(torch.randint(0, nnz + 1, (n,), generator=g)).values
            off[0] = 0
        off = off.to(dt)
        sp, dp = t.get("ids_phase", (0, 0))
        osp, odp = t.get("off_phase", (0, 0))
        e = dict(cap=cap, nnz=nnz, ids=ids, off=off, ids_src=src.take(nnz * elem, sp, data=ids) if nnz else None,
                 ids_dst=dst.take(cap * elem, dp, fill=OLD))
        if not share_offsets or k == 0:
            e["off_src"], e["off_dst"] = src.take(n * elem, osp, data=off), dst.take(bucket * elem, odp, fill=OLD)
        lay.append(e)
    src_t, want = src.build(), dst.build()
    src_d, dst_d = src_t.to(dev), want.to(dev)
    assert src_d.data_ptr() % 16 == 0 and dst_d.data_ptr() % 16 == 0
    sb, db = src_d.data_ptr(), dst_d.data_ptr()
    want[xd:xd + n * m_den * 4] = X.view(torch.uint8).reshape(-1)
    ids_segs, off_segs = [], []
    for e in lay:
        cap, nnz = e["cap"], e["nnz"]
        at = e["ids_dst"] + (cap - nnz) * elem
        want[at:at + nnz * elem] = e["ids"].view(torch.uint8)
        ids_segs.append((db + e["ids_dst"], sb + e["ids_src"] if nnz else 0, nnz, cap))      # (nothing to copy: a null source)
        if "off_dst" in e:
            want[e["off_dst"]:e["off_dst"] + bucket * elem] = want_offsets(e["off"], n, bucket, nnz, cap, dt).view(torch.uint8)
            off_segs.append((db + e["off_dst"], sb + e["off_src"], nnz, cap))
    assert _stage((db + xd, sb + xs, n * m_den * 4), ids_segs, off_segs, n, bucket, elem) == 0
    torch.cuda.synchronize()
    got = dst_d.cpu()
    assert torch.equal(got, want), "first differing byte at %d" % int((got != want).nonzero()[0])


@pytest.mark.parametrize("elem", (4, 8))
@pytest.mark.parametrize("n", (1, 7, 8))
def test_every_nnz_and_every_n(elem, n):
    """bucket 8, Lcap 24: nnz in {0, 1, Lcap - 1, Lcap} (shift 24, 23, 1, 0), n in {1, bucket - 1, bucket}"""
    _run(elem, 8, n, [dict(cap=24, nnz=z) for z in (0, 1, 23, 24)], seed=n)


@pytest.mark.parametrize("elem", (4, 8))
def test_every_source_and_destination_phase(elem):
    """sources and static buffers at every 4-byte phase modulo 16, against each other; the shifted ids destination adds its own phase
    (shift = 8 with int32 is 32 bytes, 21 - 13; the odd caps below give the others); bucket 37: 16-byte stores with words on both sides"""
    tables = []
    for sp in (0, 4, 8, 12):
        for dp in (0, 4, 8, 12):
            k = len(tables)
            tables.append(dict(cap=21 + k % 4, nnz=13 + k % 3, ids_phase=(sp, dp), off_phase=(dp, sp)))
    _run(elem, 37, 30, tables, seed=elem, x_phase=(4, 8))
    _run(elem, 37, 37, tables[:5], seed=elem + 1, x_phase=(12, 4))


@pytest.mark.parametrize("elem", (4, 8))
def test_offsets_outside_the_request_are_clamped(elem):
    """negative offsets and offsets above nnz: every static offset stays inside [shift, cap]"""
    off = torch.tensor([-5, 0, 3, 100, 7, -1, 10, 11, 2 ** 31 - 1, -2 ** 31])
    _run(elem, 16, 10, [dict(cap=48, nnz=10, off=off), dict(cap=48, nnz=0, off=off), dict(cap=16, nnz=16, off=off)], seed=3)
    if elem == 8:
        big = torch.tensor([2 ** 40, -2 ** 40, 1, 2 ** 32 + 1])       # (the high word decides)
        _run(8, 4, 4, [dict(cap=12, nnz=5, off=big)], seed=4)


@pytest.mark.parametrize("elem", (4, 8))
def test_more_segments_than_one_launch_and_more_than_one_block(elem):
    """40 tables: 1 + 40 + 40 segments, two launches; one table of 3000 lookups in a bucket of 700 bags: several blocks per segment"""
    tables = [dict(cap=9 + k % 5, nnz=(k * 7) % (9 + k % 5 + 1), ids_phase=(4 * (k % 4), 4 * ((k // 4) % 4))) for k in range(40)]
    _run(elem, 3, 2, tables, seed=5)
    _run(elem, 700, 651, [dict(cap=3000, nnz=2999, ids_phase=(4, 0)), dict(cap=3000, nnz=1501, off_phase=(8, 4))], seed=6)


def test_one_offsets_tensor_for_all_tables():
    _run(8, 8, 5, [dict(cap=24, nnz=11) for _ in range(3)], seed=7, share_offsets=True)


def test_bad_arguments_are_refused_before_anything_is_launched():
    from dlrm_amd import _lib
    dev = torch.device("cuda:0")
    a = torch.arange(64, dtype=torch.int32, device=dev)
    b = torch.full((64,), 7, dtype=torch.int32, device=dev)
    keep = b.clone()
    A, B = a.data_ptr(), b.data_ptr()
    E_ARG, E_ALIGN = -1, -2
    ok_ids, ok_off = [(B, A, 4, 8)], [(B + 128, A, 4, 8)]
    assert _stage((0, 0, 0), [], [], 0, 1, 4) == 0                                  # nothing at all: no launch
    assert _stage((0, 0, 0), ok_ids, ok_off, 2, 4, 2) == E_ARG                      # idx_bytes
    assert _stage((0, 0, 0), ok_ids, ok_off, 5, 4, 4) == E_ARG                      # n > bucket
    assert _stage((0, 0, 0), ok_ids, ok_off, -1, 4, 4) == E_ARG and _stage((0, 0, 0), ok_ids, ok_off, 0, 0, 4) == E_ARG
    assert _stage((0, 0, 0), [(B, A, 9, 8)], ok_off, 2, 4, 4) == E_ARG              # nnz > cap
    assert _stage((0, 0, 0), [(B, A, -1, 8)], ok_off, 2, 4, 4) == E_ARG             # nnz < 0
    assert _stage((0, 0, 0), ok_ids, [(B + 128, A, 9, 8)], 2, 4, 4) == E_ARG
    assert _stage((0, 0, 0), ok_ids, [(B + 128, A, 4, 2 ** 31)], 2, 4, 4) == E_ARG  # a cap an int32 offset cannot hold
    assert _stage((0, 0, 0), [(B, 0, 4, 8)], ok_off, 2, 4, 4) == E_ARG              # ids to copy, no source
    assert _stage((0, 0, 0), [(0, A, 4, 8)], ok_off, 2, 4, 4) == E_ARG              # no destination
    assert _stage((0, 0, 0), ok_ids, [(B + 128, 0, 4, 8)], 2, 4, 4) == E_ARG        # n offsets to read, no source
    assert _stage((0, 0, 0), ok_ids, [(0, A, 4, 8)], 2, 4, 4) == E_ARG
    assert _stage((B, 0, 16), [], [], 1, 4, 4) == E_ARG and _stage((0, A, 16), [], [], 1, 4, 4) == E_ARG and _stage((B, A, -4), [], [], 1, 4, 4) == E_ARG
    assert _stage((B + 2, A, 16), [], [], 1, 4, 4) == E_ALIGN and _stage((B, A + 1, 16), [], [], 1, 4, 4) == E_ALIGN
    assert _stage((B, A, 6), [], [], 1, 4, 4) == E_ALIGN
    assert _stage((0, 0, 0), [(B + 2, A, 4, 8)], ok_off, 2, 4, 4) == E_ALIGN and _stage((0, 0, 0), [(B, A + 2, 4, 8)], ok_off, 2, 4, 4) == E_ALIGN
    assert _stage((0, 0, 0), ok_ids, [(B + 130, A, 4, 8)], 2, 4, 4) == E_ALIGN and _stage((0, 0, 0), ok_ids, [(B + 128, A + 2, 4, 8)], 2, 4, 4) == E_ALIGN
    torch.cuda.synchronize()
    assert torch.equal(b, keep)                                                     # nothing was written by any refused call
    # nnz == 0 with a null ids source and n == 0 with a null offsets source are well-formed
    assert _stage((0, 0, 0), [(B, 0, 0, 8)], [(B + 128, 0, 0, 8)], 0, 4, 4) == 0
    torch.cuda.synchronize()
    assert torch.equal(b[:32], keep[:32]) and b[32:36].tolist() == [8, 8, 8, 8] and torch.equal(b[36:], keep[36:])
    with pytest.raises(RuntimeError, match="DLRM_E_ARG"):
        _lib.check(-1, "dlrm_stage_ragged")
