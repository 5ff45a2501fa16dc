"""Host side of the fused lookup + interaction forward over quantised tables (csrc/interact_quant.hip): the three entry points exist in
the library, in the bindings and in the header, and dlrm_interact_gather_quant_ok (host only, no device needed) answers as documented."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dlrm_interact_gather_quant_ok", "dlrm_interact_fwd_gather_quant", "dlrm_emb_fwd_quant_pred")


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
    # dlrm_emb_fwd_quant_pred = dlrm_emb_fwd_quant's arguments + (pred_flag, pred_nonzero) in front of the stream
    plain, pred = _lib.SIGNATURES["dlrm_emb_fwd_quant"][1], _lib.SIGNATURES["dlrm_emb_fwd_quant_pred"][1]
    assert pred == plain[:-1] + [C.c_void_p, C.c_int] + plain[-1:]
    assert len(_lib.SIGNATURES["dlrm_interact_fwd_gather_quant"][1]) == 18
    assert _lib.EXPECTED_ABI == 17          # symbols added, no signature changed


@pytest.mark.parametrize("F,D,bits,want", [(27, 128, 8, 1), (27, 128, 4, 1), (2, 128, 8, 1),
                                           (27, 64, 8, 0), (27, 128, 16, 0), (28, 128, 8, 0), (0, 128, 8, 0)])
def test_gather_quant_ok(lib, F, D, bits, want):
    fn = lib.dlrm_interact_gather_quant_ok
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int]
    assert fn(F, D, bits) == want


def test_gather_quant_ok_follows_gather_ok(lib):
    """1 for every F that dlrm_interact_gather_ok(F, 128) accepts, at both widths"""
    q, g = lib.dlrm_interact_gather_quant_ok, lib.dlrm_interact_gather_ok
    q.restype, q.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int]
    g.restype, g.argtypes = C.c_int, [C.c_int, C.c_int]
    for F in range(-1, 70):
        for bits in (4, 8):
            assert q(F, 128, bits) == g(F, 128), (F, bits)


def test_model_attribute_exists_and_is_a_bool():
    import numpy as np
    import dlrm_amd
    from dlrm_amd import dlrm_net
    model = dlrm_amd.DLRM_Net(8, np.asarray([5, 6]), np.asarray([4, 8]), np.asarray([8 + 3, 1]), "dot")
    assert model.fuse_quant_interact is dlrm_net.FUSE_QUANT_INTERACT_DEFAULT and isinstance(model.fuse_quant_interact, bool)
