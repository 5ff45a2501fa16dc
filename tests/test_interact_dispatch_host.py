"""The refusals of the interaction entry points (csrc/interact.hip: plan_fwd / plan_bwd and the entry points' own pre-checks), CPU only.

Every call of the table returns BEFORE anything is launched, so it can be made with fake addresses (the checks look at NULL-ness and
alignment only, as the GEMM route queries of tests/gemm_route_cases.py do) on a machine without a GPU.  The codes were recorded from the
library as it was before the checks moved into the plan functions: the order of the checks — which one fails FIRST — is pinned with them.
"""
from typing import NamedTuple

import pytest

E_ARG, E_RANGE, E_MODE = -1, -3, -4
BASE = 0x10000000          # fake device addresses: multiples of 16 unless a case moves one


class Call(NamedTuple):
    name: str
    entry: str              # fwd | bwd | fwd_gather | bwd_gather | fwd_pred | bwd_pred | bwd_sgd
    expect: int
    B: int = 9
    F: int = 4
    D: int = 128
    mode: int = 0
    idx_bits: int = 64
    ldr: int = 0            # 0: the output width rounded up to 4
    r_off: int = 0          # bytes added to the address of R / dR
    feat_null: int = -1     # this feature's pointer is NULL
    dfeat_null: int = -1
    feat_lists: bool = True     # False: the feature pointer LIST is NULL
    gather: str = "tables"  # which features are gathered: "tables" = 1 .. F-1, "all" = 0 .. F-1, "none" = the lists hold only NULLs
    lists: tuple = ("idx", "off", "rows")     # which of the three gather lists are passed at all
    off_null: int = -1      # this gathered feature's offsets pointer is NULL
    rows: int = 1000        # rows of every table
    table_ld: int = 0       # 0: D
    dfeat_ld: int = 0       # 0: D
    mask: bool = True       # bwd_sgd: the single-lookup mask is passed


def width(c: Call) -> int:
    return c.D + (c.F * (c.F + 1) // 2 if c.mode & 1 else c.F * (c.F - 1) // 2)


CALLS = [
    # ---- sizes and lists
    Call("fwd_B0", "fwd", E_ARG, B=0), Call("fwd_F0", "fwd", E_ARG, F=0), Call("fwd_D0", "fwd", E_ARG, D=0),
    Call("bwd_B_negative", "bwd", E_ARG, B=-1), Call("bwd_F0", "bwd", E_ARG, F=0), Call("bwd_D_negative", "bwd", E_ARG, D=-4),
    Call("fwd_no_feature_list", "fwd", E_ARG, feat_lists=False), Call("bwd_no_feature_list", "bwd", E_ARG, feat_lists=False),
    Call("fwd_null_feature", "fwd", E_ARG, feat_null=2), Call("bwd_null_feature", "bwd", E_ARG, feat_null=0),
    Call("bwd_null_gradient_block", "bwd", E_ARG, dfeat_null=3),
    Call("fwd_F65", "fwd", E_RANGE, F=65, D=16), Call("bwd_F65", "bwd", E_RANGE, F=65, D=16),
    Call("fwd_F65_comes_before_the_mode", "fwd", E_RANGE, F=65, D=16, mode=3),
    # ---- modes
    Call("fwd_mode3", "fwd", E_MODE, mode=3), Call("fwd_mode4_is_backward_only", "fwd", E_MODE, mode=4),
    Call("fwd_mode_negative", "fwd", E_MODE, mode=-1),
    Call("bwd_mode8", "bwd", E_MODE, mode=8), Call("bwd_mode3_relu", "bwd", E_MODE, mode=3 | 4), Call("bwd_mode3", "bwd", E_MODE, mode=3),
    Call("fwd_mode_comes_before_the_pitch", "fwd", E_MODE, mode=3, ldr=4),
    # ---- the pitch of R / dR
    Call("fwd_ldr_short", "fwd", E_ARG, ldr=128 + 5), Call("fwd_ldr_short_self", "fwd", E_ARG, mode=1, ldr=128 + 9),
    Call("bwd_ldr_short", "bwd", E_ARG, D=16, ldr=16 + 5), Call("fwd_gather_ldr_short", "fwd_gather", E_ARG, ldr=128),
    # ---- the gather lists
    Call("fwd_gather_no_index_list", "fwd_gather", E_ARG, lists=("off", "rows")),
    Call("fwd_gather_no_offsets_list", "fwd_gather", E_ARG, lists=("idx", "rows")),
    Call("bwd_gather_no_rows_list", "bwd_gather", E_ARG, lists=("idx", "off")),
    Call("fwd_pred_index_without_offsets", "fwd_pred", E_ARG, lists=("idx", "rows")),
    Call("bwd_pred_index_without_rows", "bwd_pred", E_ARG, lists=("idx", "off")),
    Call("fwd_gather_null_offsets_of_a_table", "fwd_gather", E_ARG, off_null=2),
    Call("bwd_gather_null_offsets_of_a_table", "bwd_gather", E_ARG, off_null=1),
    Call("fwd_gather_idx_bits16", "fwd_gather", E_MODE, idx_bits=16), Call("bwd_gather_idx_bits16", "bwd_gather", E_MODE, idx_bits=16),
    Call("fwd_pred_idx_bits16", "fwd_pred", E_MODE, idx_bits=16), Call("bwd_pred_idx_bits16", "bwd_pred", E_MODE, idx_bits=16),
    Call("bwd_sgd_idx_bits16", "bwd_sgd", E_MODE, idx_bits=16),
    Call("fwd_gather_rows0", "fwd_gather", E_ARG, rows=0), Call("bwd_gather_rows_negative", "bwd_gather", E_ARG, rows=-5),
    Call("fwd_gather_rows_2p32", "fwd_gather", E_RANGE, rows=1 << 32), Call("bwd_gather_rows_2p32", "bwd_gather", E_RANGE, rows=1 << 32),
    Call("fwd_gather_rows_come_before_the_shape", "fwd_gather", E_RANGE, D=64, rows=1 << 32),
    # ---- gathered features outside the D = 128 image kernels
    Call("fwd_gather_D64", "fwd_gather", E_MODE, D=64), Call("bwd_gather_D64", "bwd_gather", E_MODE, D=64),
    Call("fwd_pred_gather_D64", "fwd_pred", E_MODE, D=64), Call("bwd_pred_gather_D16", "bwd_pred", E_MODE, D=16),
    Call("fwd_gather_F28", "fwd_gather", E_MODE, F=28), Call("bwd_gather_F28", "bwd_gather", E_MODE, F=28),
    Call("fwd_gather_R_misaligned", "fwd_gather", E_MODE, r_off=4), Call("bwd_gather_dR_misaligned", "bwd_gather", E_MODE, r_off=8),
    Call("fwd_gather_ldr_odd", "fwd_gather", E_MODE, ldr=128 + 6 + 1), Call("bwd_gather_ldr_odd", "bwd_gather", E_MODE, ldr=128 + 6 + 3),
    Call("fwd_gather_table_pitch_odd", "fwd_gather", E_MODE, table_ld=130),
    Call("bwd_gather_gradient_pitch_odd", "bwd_gather", E_MODE, dfeat_ld=130),
    Call("bwd_gather_dR_row_fills_the_image", "bwd_gather", E_MODE, F=27, ldr=512),
    Call("bwd_gather_dR_row_beyond_the_image", "bwd_gather", E_MODE, F=27, ldr=516),
    Call("bwd_sgd_dR_row_fills_the_image", "bwd_sgd", E_MODE, F=27, ldr=512),
    # ---- the update inside the backward
    Call("bwd_sgd_no_mask", "bwd_sgd", E_ARG, mask=False),
    Call("bwd_sgd_mask_without_gather_lists", "bwd_sgd", E_ARG, lists=()),
    Call("bwd_sgd_feature0_gathered", "bwd_sgd", E_ARG, gather="all"),
    Call("bwd_sgd_a_plain_feature", "bwd_sgd", E_ARG, gather="none"),
    Call("bwd_sgd_table_pitch", "bwd_sgd", E_ARG, table_ld=132),
    Call("bwd_sgd_gradient_pitch_2p30", "bwd_sgd", E_RANGE, dfeat_ld=1 << 30),
    Call("bwd_sgd_gradient_pitch_negative", "bwd_sgd", E_RANGE, dfeat_ld=-4),
    Call("bwd_sgd_B_2p32", "bwd_sgd", E_RANGE, B=1 << 32),
    Call("bwd_sgd_D64", "bwd_sgd", E_MODE, D=64),
    # ---- the generic kernels' LDS
    Call("fwd_generic_lds", "fwd", E_RANGE, F=64, D=512), Call("bwd_generic_lds", "bwd", E_RANGE, F=64, D=512),
    Call("fwd_pred_generic_lds", "fwd_pred", E_RANGE, F=64, D=512, gather="none", lists=()),
    Call("bwd_generic_lds_F33", "bwd", E_RANGE, F=33, D=300),
]


def run(c: Call) -> int:
    from dlrm_amd import _lib
    lib = _lib.load()
    F = max(c.F, 1)
    tld = c.table_ld or c.D
    feat = [0 if f == c.feat_null else BASE + 0x100000 * f for f in range(F)]
    feat_ld = [c.D] + [tld] * (F - 1)
    dfeat = [0 if f == c.dfeat_null else 3 * BASE + 0x100000 * f for f in range(F)]
    dfeat_ld = [c.dfeat_ld or c.D] * F
    gathered = [c.gather == "all" or (c.gather == "tables" and f > 0) for f in range(F)]
    gidx = [5 * BASE + 0x1000 * f if g else 0 for f, g in enumerate(gathered)]
    goff = [6 * BASE + 0x1000 * f if g and f != c.off_null else 0 for f, g in enumerate(gathered)]
    rows = [c.rows if g else 0 for g in gathered]
    p = _lib.ptr_array(feat) if c.feat_lists else None
    lists = (_lib.ptr_array(gidx) if "idx" in c.lists else None, _lib.ptr_array(goff) if "off" in c.lists else None,
             _lib.i64_array(rows) if "rows" in c.lists else None)
    ldr = c.ldr or ((width(c) + 3) & ~3)
    R, err, flag, mask = 2 * BASE + c.r_off, 7 * BASE, 8 * BASE, 9 * BASE
    head = (c.B, c.F, c.D, p, _lib.i64_array(feat_ld))
    grads = (_lib.ptr_array(dfeat), _lib.i64_array(dfeat_ld))
    if c.entry == "fwd":
        return lib.dlrm_interact_fwd(*head, c.mode, R, ldr, None)
    if c.entry == "bwd":
        return lib.dlrm_interact_bwd(*head, c.mode, R, ldr, *grads, None)
    if c.entry == "fwd_gather":
        return lib.dlrm_interact_fwd_gather(*head, *lists, c.idx_bits, c.mode, R, ldr, err, None)
    if c.entry == "bwd_gather":
        return lib.dlrm_interact_bwd_gather(*head, *lists, c.idx_bits, c.mode, R, ldr, *grads, err, None)
    if c.entry == "fwd_pred":
        return lib.dlrm_interact_fwd_pred(*head, *lists, c.idx_bits, c.mode, R, ldr, err, flag, 0, None)
    if c.entry == "bwd_pred":
        return lib.dlrm_interact_bwd_pred(*head, *lists, c.idx_bits, c.mode, R, ldr, *grads, err, flag, 0, None)
    assert c.entry == "bwd_sgd", c.entry
    return lib.dlrm_interact_bwd_gather_sgd(*head, *lists, c.idx_bits, c.mode, R, ldr, *grads, mask if c.mask else None, 0.1, None, err,
                                            flag, 0, None)


def test_case_names_are_unique_and_every_entry_point_is_asked():
    names = [c.name for c in CALLS]
    assert len(set(names)) == len(names)
    assert {c.entry for c in CALLS} == {"fwd", "bwd", "fwd_gather", "bwd_gather", "fwd_pred", "bwd_pred", "bwd_sgd"}
    assert {c.expect for c in CALLS} == {E_ARG, E_RANGE, E_MODE}


@pytest.mark.parametrize("c", CALLS, ids=[c.name for c in CALLS])
def test_refusal_code(c):
    assert run(c) == c.expect


def test_gather_shapes():
    """dlrm_interact_gather_ok: D = 128 and a dR row (with self pairs) that fits the 2 KiB image of the gather backward, F <= 27"""
    from dlrm_amd import _lib
    lib = _lib.load()
    ok = [(F, D) for D in (16, 64, 127, 128, 129, 256) for F in range(0, 34) if lib.dlrm_interact_gather_ok(F, D)]
    assert ok == [(F, 128) for F in range(1, 28)]
