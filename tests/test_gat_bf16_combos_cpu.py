"""CPU suite: the one-sweep GAT under attention dropout on bf16 tables (gaib_gat_forward_fused_drop_bf16 /
gaib_gat_backward_fused_drop_bf16) is exported, bound and wrapped.  tests/test_abi.py holds the ctypes table against
include/gaib.h; no compute calls here (no GPU)."""
import ctypes

from graphaibench_amd import capi

NEW = ("gaib_gat_forward_fused_drop_bf16", "gaib_gat_backward_fused_drop_bf16")


def test_library_exports_the_two_entry_points():
    lib = ctypes.CDLL(str(capi.LIB_PATH))
    for name in NEW:
        assert hasattr(lib, name), name


def test_signatures_are_the_drop_rows_on_bf16_table_pointers():
    """argument order of the _drop calls; the table positions (h; feat and grad) are pointers there and here (uint16_t* in the
    header: raw bf16 bits), every scalar keeps its type and place"""
    for name in NEW:
        assert capi.SIGNATURES[name] == capi.SIGNATURES[name[: -len("_bf16")]], name
    res, args = capi.SIGNATURES[NEW[0]]
    assert res is ctypes.c_int and len(args) == 14 and args[4] is ctypes.c_void_p and args[11] is ctypes.c_uint64
    res, args = capi.SIGNATURES[NEW[1]]
    assert res is ctypes.c_int and len(args) == 17 and args[4] is ctypes.c_void_p and args[5] is ctypes.c_void_p
    assert args[13] is ctypes.c_uint64


def test_context_wrappers_exist():
    for name in ("gat_forward_fused_drop_bf16", "gat_backward_fused_drop_bf16"):
        assert callable(getattr(capi.Context, name)), name


def test_error_path_without_gpu():
    """the argument checks come before the device, as in every entry point"""
    lib = capi.load()
    assert lib.gaib_gat_forward_fused_drop_bf16(None, None, 64, 8, None, None, None, 0.2, 0, 0.3, 1.0, 1, None, None) != 0
    assert b"NULL" in lib.gaib_last_error()
    assert lib.gaib_gat_backward_fused_drop_bf16(None, None, 64, 8, None, None, None, None, None, None, 0.2, 0.3, 1.0, 1, None, None,
                                                 None) != 0
    assert b"NULL" in lib.gaib_last_error()
