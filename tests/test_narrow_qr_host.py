"""Host side of the fused lookup + interaction kernels over quotient-remainder tables of D = 16 / 32 / 64 (csrc/interact_narrow_qr.hip): the
three entry points exist in the library, in the bindings and in the header with the signatures of their D = 128 siblings, the *_ok function
(host only, no device needed) answers as documented, the D = 128 QR sibling still refuses the narrow widths, no default of the model changed
and the launcher has no new flag."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dlrm_interact_gather_narrow_qr_ok", "dlrm_interact_fwd_gather_narrow_qr", "dlrm_interact_bwd_gather_narrow_qr")


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
    sig = _lib.SIGNATURES
    # the argument lists of the D = 128 QR entry points, type for type: 20 and 24 arguments, launch predicate included
    assert sig["dlrm_interact_fwd_gather_narrow_qr"] == sig["dlrm_interact_fwd_gather_qr"]
    assert sig["dlrm_interact_bwd_gather_narrow_qr"] == sig["dlrm_interact_bwd_gather_qr"]
    assert sig["dlrm_interact_gather_narrow_qr_ok"] == sig["dlrm_interact_gather_qr_ok"]
    assert len(sig["dlrm_interact_fwd_gather_narrow_qr"][1]) == 20
    assert len(sig["dlrm_interact_bwd_gather_narrow_qr"][1]) == 24
    assert _lib.EXPECTED_ABI == 17          # symbols added, no signature changed


def test_header_declarations_match_their_siblings():
    """the C parameter lists, names and all, are those of the D = 128 siblings"""
    header = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()

    def params(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1)).strip()
    assert params("dlrm_interact_fwd_gather_narrow_qr") == params("dlrm_interact_fwd_gather_qr")
    assert params("dlrm_interact_bwd_gather_narrow_qr") == params("dlrm_interact_bwd_gather_qr")
    assert params("dlrm_interact_gather_narrow_qr_ok") == params("dlrm_interact_gather_qr_ok")


def test_the_ok_function_equals_the_narrow_one_everywhere(lib):
    n = lib.dlrm_interact_gather_narrow_ok
    q = lib.dlrm_interact_gather_narrow_qr_ok
    n.restype, n.argtypes = C.c_int, [C.c_int, C.c_int]
    q.restype, q.argtypes = C.c_int, [C.c_int, C.c_int]
    for F, D in ((2, 16), (27, 16), (27, 32), (27, 64), (32, 64), (1, 16)):
        assert q(F, D) == 1, (F, D)
    for F in range(-2, 70):
        for D in range(-4, 140):
            assert q(F, D) == n(F, D) == int(D in (16, 32, 64) and 1 <= F <= 32), (F, D)


def test_the_d128_qr_sibling_still_refuses_the_narrow_widths(lib):
    q = lib.dlrm_interact_gather_qr_ok
    q.restype, q.argtypes = C.c_int, [C.c_int, C.c_int]
    for F in (2, 16, 17, 27):
        for D in (16, 32, 64):
            assert q(F, D) == 0, (F, D)
        assert q(F, 128) == 1, F
    # ... and the narrow one D = 128
    assert lib.dlrm_interact_gather_narrow_qr_ok(27, 128) == 0


def test_model_defaults_are_unchanged():
    import numpy as np
    import dlrm_amd
    assert dlrm_amd.DLRM_Net.fuse_narrow_interact is False
    assert dlrm_amd.DLRM_Net.fuse_qr_interact is False
    model = dlrm_amd.DLRM_Net(16, np.asarray([500, 6]), np.asarray([4, 16]), np.asarray([16 + 3, 1]), "dot", qr_flag=True, qr_operation="mult",
                              qr_collisions=4, qr_threshold=200)
    assert model._has_qr(model.emb_l)
    assert model.fuse_narrow_interact is False and model.fuse_qr_interact is False


def test_launcher_has_no_new_flag_and_both_help_texts_name_the_combination():
    from dlrm_amd import launch
    ap = launch.build_parser()
    flags = sorted(s for a in ap._actions for s in a.option_strings if s.startswith("--"))
    assert flags == sorted(["--help", "--reference", "--device-tables", "--bf16-tables", "--bf16-seed", "--bf16-fuse-interact",
                            "--qr-fuse-interact", "--narrow-fuse-interact", "--fused-adagrad"])
    text = {s: a.help for a in ap._actions for s in a.option_strings}
    assert "--narrow-fuse-interact" in text["--qr-fuse-interact"] and "16 / 32 / 64" in text["--qr-fuse-interact"]
    assert "--qr-fuse-interact" in text["--narrow-fuse-interact"] and "--qr-flag" in text["--narrow-fuse-interact"]
    a = ap.parse_args(["--narrow-fuse-interact", "--qr-fuse-interact"])
    assert a.narrow_fuse_interact and a.qr_fuse_interact
