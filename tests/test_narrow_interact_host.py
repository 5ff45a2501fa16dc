"""Host side of the fused lookup + interaction kernels over plain fp32 tables of D = 16 / 32 / 64 (csrc/interact_narrow.hip): the three entry
points exist in the library, in the bindings and in the header, dlrm_interact_gather_narrow_ok (host only, no device needed) answers as
documented, the D = 128 siblings still refuse D = 64, the model's opt-in attribute defaults to off and the launcher knows its flag."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dlrm_interact_gather_narrow_ok", "dlrm_interact_fwd_gather_narrow", "dlrm_interact_bwd_gather_narrow")


@pytest.fixture(scope="module")
def lib():
    from dlrm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return C.CDLL(_lib.LIB_PATH)          # plain dlopen: no device is touched


def test_library_exports_the_new_symbols(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_bindings_and_header_list_them():
    from dlrm_amd import _lib
    header = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert len(_lib.SIGNATURES["dlrm_interact_fwd_gather_narrow"][1]) == 17
    assert len(_lib.SIGNATURES["dlrm_interact_bwd_gather_narrow"][1]) == 21
    # the arguments of the bf16 siblings, type for type
    assert _lib.SIGNATURES["dlrm_interact_fwd_gather_narrow"] == _lib.SIGNATURES["dlrm_interact_fwd_gather_bf16"]
    assert _lib.SIGNATURES["dlrm_interact_bwd_gather_narrow"] == _lib.SIGNATURES["dlrm_interact_bwd_gather_bf16"]
    assert _lib.EXPECTED_ABI == 17          # symbols added, no signature changed


def test_gather_narrow_ok(lib):
    """1 iff D in {16, 32, 64} and 1 <= F <= 32"""
    q = lib.dlrm_interact_gather_narrow_ok
    q.restype, q.argtypes = C.c_int, [C.c_int, C.c_int]
    for F, D in ((2, 16), (27, 16), (27, 32), (27, 64), (32, 64)):
        assert q(F, D) == 1, (F, D)
    for D in (0, 8, 48, 128):
        assert q(27, D) == 0, D
    for F in (0, 33):
        for D in (16, 32, 64):
            assert q(F, D) == 0, (F, D)
    for F in range(-2, 70):
        for D in range(-4, 140, 4):
            assert q(F, D) == int(D in (16, 32, 64) and 1 <= F <= 32), (F, D)


def test_the_d128_siblings_still_refuse_d64(lib):
    for name in ("dlrm_interact_gather_ok", "dlrm_interact_gather_bf16_ok", "dlrm_interact_gather_qr_ok"):
        q = getattr(lib, name)
        q.restype, q.argtypes = C.c_int, [C.c_int, C.c_int]
        for F in (2, 16, 17, 27):
            assert q(F, 64) == 0, (name, F)
            assert q(F, 128) == 1, (name, F)
    q = lib.dlrm_interact_gather_quant_ok
    q.restype, q.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int]
    for bits in (4, 8):
        assert q(27, 64, bits) == 0 and q(27, 128, bits) == 1


def test_model_attribute_is_off_by_default():
    import numpy as np
    import dlrm_amd
    assert dlrm_amd.DLRM_Net.fuse_narrow_interact is False
    model = dlrm_amd.DLRM_Net(16, np.asarray([5, 6]), np.asarray([4, 16]), np.asarray([16 + 3, 1]), "dot")
    assert model.fuse_narrow_interact is False


def test_launcher_parses_the_flag():
    from dlrm_amd import launch
    ap = launch.build_parser()
    assert ap.parse_args([]).narrow_fuse_interact is False
    assert ap.parse_args(["--narrow-fuse-interact"]).narrow_fuse_interact is True
