"""CPU suite: the window forms of the dropped one-sweep GAT calls (gaib_gat_forward_fused_drop_win /
gaib_gat_backward_fused_drop_win: the unit a dropped call on rows wider than 128 columns is made of) are exported by the library
and stand in the Python table as the _drop calls with two more c_int arguments, mask_heads and mask_head0, behind the seed
(tests/test_abi.py checks the table against include/gaib.h).  What they compute is a GPU matter: tests/test_gpu_gat_wide_drop.py."""
import ctypes as C

from graphaibench_amd import capi


def test_library_exports_the_two_window_entries():
    lib = C.CDLL(str(capi.LIB_PATH))
    assert hasattr(lib, "gaib_gat_forward_fused_drop_win") and hasattr(lib, "gaib_gat_backward_fused_drop_win")


def test_signatures_are_the_drop_calls_with_the_window():
    for name, seed_at in (("gaib_gat_forward_fused_drop", 11), ("gaib_gat_backward_fused_drop", 13)):
        res, args = capi.SIGNATURES[name]
        res_w, args_w = capi.SIGNATURES[name + "_win"]
        assert res_w is res is C.c_int
        assert args[seed_at] is C.c_uint64
        assert args_w == args[:seed_at + 1] + [C.c_int, C.c_int] + args[seed_at + 1:], name
    for name in ("gat_forward_fused_drop_win", "gat_backward_fused_drop_win"):
        assert callable(getattr(capi.Context, name))
