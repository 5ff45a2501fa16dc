"""Host side of the fused lookup + interaction kernels over quotient-remainder tables (csrc/interact_qr.hip): the five entry points exist in
the library, in the bindings and in the header, dlrm_interact_gather_qr_ok (host only, no device needed) answers as documented, the model's
opt-in attribute defaults to off and the launcher knows its flag."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dlrm_interact_gather_qr_ok", "dlrm_interact_fwd_gather_qr", "dlrm_interact_bwd_gather_qr", "dlrm_emb_fwd_qr_pred",
               "dlrm_emb_qr_bwd_split_pred")


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
    # the _pred entry points = the plain ones' arguments + (pred_flag, pred_nonzero) in front of the stream
    for name in ("dlrm_emb_fwd_qr", "dlrm_emb_qr_bwd_split"):
        plain, pred = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name + "_pred"][1]
        assert pred == plain[:-1] + [C.c_void_p, C.c_int] + plain[-1:], name
    # the bf16 entry points' arguments + weight_r_host, collisions_host, op
    assert len(_lib.SIGNATURES["dlrm_interact_fwd_gather_qr"][1]) == len(_lib.SIGNATURES["dlrm_interact_fwd_gather_bf16"][1]) + 3 == 20
    assert len(_lib.SIGNATURES["dlrm_interact_bwd_gather_qr"][1]) == len(_lib.SIGNATURES["dlrm_interact_bwd_gather_bf16"][1]) + 3 == 24
    assert _lib.EXPECTED_ABI == 17          # symbols added, no signature changed


def test_gather_qr_ok_follows_gather_ok(lib):
    """D == 128 && dlrm_interact_gather_ok(F, D); it takes no collision count, so it cannot depend on one"""
    q, g = lib.dlrm_interact_gather_qr_ok, lib.dlrm_interact_gather_ok
    q.restype, q.argtypes = C.c_int, [C.c_int, C.c_int]
    g.restype, g.argtypes = C.c_int, [C.c_int, C.c_int]
    for F in range(-1, 70):
        assert q(F, 128) == g(F, 128), F
        for D in (4, 16, 64, 127, 132, 256):
            assert q(F, D) == 0, (F, D)
    assert q(27, 128) == 1 and q(2, 128) == 1 and q(28, 128) == 0 and q(0, 128) == 0


def test_model_attribute_is_off_by_default():
    import numpy as np
    import dlrm_amd
    assert dlrm_amd.DLRM_Net.fuse_qr_interact is False
    model = dlrm_amd.DLRM_Net(8, np.asarray([5, 6]), np.asarray([4, 8]), np.asarray([8 + 3, 1]), "dot")
    assert model.fuse_qr_interact is False
    model = dlrm_amd.DLRM_Net(8, np.asarray([300, 6]), np.asarray([4, 8]), np.asarray([8 + 3, 1]), "dot", qr_flag=True, qr_threshold=200,
                              qr_collisions=4)
    assert model._has_qr(model.emb_l) and model.fuse_qr_interact is False


def test_launcher_parses_the_flag():
    from dlrm_amd import launch
    ap = launch.build_parser()
    assert ap.parse_args([]).qr_fuse_interact is False
    assert ap.parse_args(["--qr-fuse-interact"]).qr_fuse_interact is True
