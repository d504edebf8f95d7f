"""CPU suite: the shape rule of the one-sweep GAT on rows wider than 128 columns (gaib_gat_fused_slabs: a pure function, no
context, no device), its place in the Python table, and the 0|1 switch behind GAIB_GAT_WIDE as the context reads it.  The
refusal of a bad value by a running process is a GPU test (tests/test_gpu_gat_wide.py)."""
import ctypes as C

from graphaibench_amd import capi, layers as L

# (len, heads) -> (w, S); S = 0: no one-sweep form
TABLE = {
    (128, 8): (128, 1), (256, 8): (128, 2), (256, 2): (128, 2), (256, 32): (128, 2), (256, 64): (64, 4), (512, 8): (128, 4),
    (1024, 16): (128, 8), (384, 24): (128, 3), (192, 6): (64, 3), (96, 3): (32, 3), (160, 5): (32, 5),
    (256, 1): None, (200, 8): None, (64, 3): None, (256, 3): None,
}


def narrow_shape(length, heads):
    """where the one-sweep kernels apply today: len 32 / 64 / 128, 1, 2, 4, 8 or 16 heads of at least 4 columns"""
    return length in (32, 64, 128) and heads in (1, 2, 4, 8, 16) and heads * 4 <= length


def test_library_and_table_hold_the_symbol():
    lib = C.CDLL(str(capi.LIB_PATH))
    assert hasattr(lib, "gaib_gat_fused_slabs")
    sig = capi.SIGNATURES["gaib_gat_fused_slabs"]
    assert sig[0] is C.c_int and len(sig[1]) == 3 and sig[1][:2] == [C.c_int, C.c_int]
    assert callable(capi.gat_fused_slabs)


def test_the_rule_returns_the_stated_answers():
    for (length, heads), want in TABLE.items():
        w, S = capi.gat_fused_slabs(length, heads)
        if want is None:
            assert S == 0, (length, heads, w, S)
        else:
            assert (w, S) == want, (length, heads, w, S)
    # the width pointer may be NULL
    assert capi.load().gaib_gat_fused_slabs(256, 8, None) == 2


def test_up_to_128_columns_it_is_the_one_sweep_cover_of_today():
    for length in range(1, 129):
        for heads in range(1, 33):
            w, S = capi.gat_fused_slabs(length, heads)
            if narrow_shape(length, heads):
                assert (w, S) == (length, 1), (length, heads, w, S)
            elif (length, heads) in TABLE and TABLE[(length, heads)] is not None:
                assert (w, S) == TABLE[(length, heads)]  # (96, 3): three slabs of 32
            elif S != 0:
                # a slab form below 128 columns: checked against the rule itself
                assert S >= 2 and w in (64, 32) and w * S == length and heads % S == 0 and narrow_shape(w, heads // S), (length, heads, w, S)
                assert not (w == 32 and length % 64 == 0 and heads % (length // 64) == 0 and narrow_shape(64, heads // (length // 64)))
            else:
                for cand in (64, 32):
                    S2 = length // cand
                    assert not (length % cand == 0 and S2 >= 2 and heads % S2 == 0 and narrow_shape(cand, heads // S2)), (length, heads)
    for bad in ((0, 1), (-128, 8), (128, 0), (256, -8)):
        assert capi.gat_fused_slabs(*bad)[1] == 0, bad


def test_wide_switch_parses():
    lib = L.load()
    assert lib.gaibl_parse_switch(b"0") == 0 and lib.gaibl_parse_switch(b"1") == 1
    for bad in (b"2", b"", b"10", b"yes", b"-1", b"1 ", None):
        assert lib.gaibl_parse_switch(bad) == -1, bad
