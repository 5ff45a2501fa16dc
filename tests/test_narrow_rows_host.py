"""Host side of the fused lookup + interaction kernels over bfloat16 and 8- / 4-bit packed tables of D = 16 / 32 / 64
(csrc/interact_narrow_rows.hip): the five entry points exist in the library, in the bindings and in the header with the signatures of their
siblings, the two *_ok functions (host only, no device needed) answer as documented, the D = 128 siblings still refuse D = 64, and no
default of the model changed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dlrm_interact_gather_narrow_bf16_ok", "dlrm_interact_gather_narrow_quant_ok", "dlrm_interact_fwd_gather_narrow_bf16",
               "dlrm_interact_bwd_gather_narrow_bf16", "dlrm_interact_fwd_gather_narrow_quant")


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
    # the argument lists of the fp32 narrow entry points, type for type: 17 and 21 arguments, launch predicate included
    assert sig["dlrm_interact_fwd_gather_narrow_bf16"] == sig["dlrm_interact_fwd_gather_narrow"]
    assert sig["dlrm_interact_bwd_gather_narrow_bf16"] == sig["dlrm_interact_bwd_gather_narrow"]
    assert len(sig["dlrm_interact_fwd_gather_narrow_bf16"][1]) == 17
    assert len(sig["dlrm_interact_bwd_gather_narrow_bf16"][1]) == 21
    # ... and of the D = 128 quantised forward
    assert sig["dlrm_interact_fwd_gather_narrow_quant"] == sig["dlrm_interact_fwd_gather_quant"]
    assert sig["dlrm_interact_gather_narrow_bf16_ok"] == sig["dlrm_interact_gather_narrow_ok"]
    assert sig["dlrm_interact_gather_narrow_quant_ok"] == sig["dlrm_interact_gather_quant_ok"]
    assert _lib.EXPECTED_ABI == 17          # symbols added, no signature changed


def test_header_declarations_match_their_siblings():
    """the C parameter lists, names and all, are those of the siblings"""
    header = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()

    def params(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1)).strip()
    assert params("dlrm_interact_fwd_gather_narrow_bf16") == params("dlrm_interact_fwd_gather_narrow")
    assert params("dlrm_interact_bwd_gather_narrow_bf16") == params("dlrm_interact_bwd_gather_narrow")
    assert params("dlrm_interact_fwd_gather_narrow_quant") == params("dlrm_interact_fwd_gather_quant")


def test_the_ok_functions(lib):
    """bf16: 1 iff dlrm_interact_gather_narrow_ok(F, D), that is D in {16, 32, 64} and 1 <= F <= 32; quant: the same and bits in {4, 8}"""
    n = lib.dlrm_interact_gather_narrow_ok
    b = lib.dlrm_interact_gather_narrow_bf16_ok
    q = lib.dlrm_interact_gather_narrow_quant_ok
    n.restype, n.argtypes = C.c_int, [C.c_int, C.c_int]
    b.restype, b.argtypes = C.c_int, [C.c_int, C.c_int]
    q.restype, q.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int]
    for F, D in ((2, 16), (27, 16), (27, 32), (27, 64), (32, 64), (1, 16)):
        assert b(F, D) == 1 and q(F, D, 4) == 1 and q(F, D, 8) == 1, (F, D)
    for F in range(-2, 70):
        for D in range(-4, 140, 4):
            rule = int(D in (16, 32, 64) and 1 <= F <= 32)
            assert n(F, D) == rule, (F, D)
            assert b(F, D) == rule, (F, D)
            for bits in (-8, 0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 32):
                assert q(F, D, bits) == int(rule and bits in (4, 8)), (F, D, bits)


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
    # ... and the narrow ones D = 128
    for bits in (4, 8):
        assert lib.dlrm_interact_gather_narrow_quant_ok(27, 128, bits) == 0
    assert lib.dlrm_interact_gather_narrow_bf16_ok(27, 128) == 0


def test_model_defaults_are_unchanged():
    import numpy as np
    import dlrm_amd
    from dlrm_amd import dlrm_net
    assert dlrm_amd.DLRM_Net.fuse_narrow_interact is False
    assert dlrm_amd.DLRM_Net.fuse_bf16_interact is False
    assert dlrm_net.FUSE_QUANT_INTERACT_DEFAULT is True
    model = dlrm_amd.DLRM_Net(16, np.asarray([5, 6]), np.asarray([4, 16]), np.asarray([16 + 3, 1]), "dot")
    assert model.fuse_narrow_interact is False and model.fuse_bf16_interact is False
    assert model.fuse_quant_interact is True


def test_launcher_has_no_new_flag_and_its_help_names_the_new_paths():
    from dlrm_amd import launch
    ap = launch.build_parser()
    flags = sorted(s for a in ap._actions for s in a.option_strings if s.startswith("--"))
    assert flags == sorted(["--help", "--reference", "--device-tables", "--bf16-tables", "--bf16-seed", "--bf16-fuse-interact",
                            "--qr-fuse-interact", "--narrow-fuse-interact", "--fused-adagrad"])
    text = {s: a.help for a in ap._actions for s in a.option_strings}
    assert "--bf16-fuse-interact" in text["--narrow-fuse-interact"] and "quantize-emb-with-bit" in text["--narrow-fuse-interact"]
    assert "--narrow-fuse-interact" in text["--bf16-fuse-interact"]
    assert "--narrow-fuse-interact" in text["--bf16-tables"]
    a = ap.parse_args(["--narrow-fuse-interact", "--bf16-tables", "nearest", "--bf16-fuse-interact"])
    assert a.narrow_fuse_interact and a.bf16_fuse_interact and a.bf16_tables == "nearest"
