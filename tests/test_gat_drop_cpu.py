"""CPU suite: the two entry points of the one-sweep GAT under attention dropout are in the Python table with the arguments
include/gaib.h declares (tests/test_abi.py checks table against header and library), and the 0|1 switch behind
GAIB_GAT_FUSED_DROP parses as the context reads it.  The context reads the variable after it has created its device context,
so the refusal of a bad value by a running process is a GPU test (tests/test_gpu_gat_drop.py)."""
import ctypes as C

from graphaibench_amd import capi, layers as L


def test_signatures_hold_the_two_entries():
    fwd = capi.SIGNATURES["gaib_gat_forward_fused_drop"]
    bwd = capi.SIGNATURES["gaib_gat_backward_fused_drop"]
    assert fwd[0] is C.c_int and bwd[0] is C.c_int
    # ctx, g, len, heads, h, alpha_l, alpha_r, eps, relu, rate, scale, seed, out, row_stats
    assert len(fwd[1]) == 14 and fwd[1][9:12] == [C.c_float, C.c_float, C.c_uint64]
    # ctx, g, len, heads, feat, grad, fwd_out, alpha_l, alpha_r, row_stats, eps, rate, scale, seed, grad_out, lgrad, rgrad
    assert len(bwd[1]) == 17 and bwd[1][10:14] == [C.c_float, C.c_float, C.c_float, C.c_uint64]
    for name in ("gat_forward_fused_drop", "gat_backward_fused_drop"):
        assert callable(getattr(capi.Context, name))


def test_library_exports_the_two_entries():
    lib = C.CDLL(str(capi.LIB_PATH))
    assert hasattr(lib, "gaib_gat_forward_fused_drop") and hasattr(lib, "gaib_gat_backward_fused_drop")


def test_fused_drop_switch_parses():
    lib = L.load()
    assert lib.gaibl_parse_switch(b"0") == 0 and lib.gaibl_parse_switch(b"1") == 1
    for bad in (b"2", b"", b"10", b"yes", b"-1", b"1 ", None):
        assert lib.gaibl_parse_switch(bad) == -1, bad
