"""CPU suite: gaib_dropout_dev is in the Python table with the arguments include/gaib.h declares, refuses a NULL context before it
touches a device, and the 0|1 switch behind GAIB_DROP_SEED_DEV parses as the context reads it.  The context reads the variable
after it has created its device context, so the refusal of a bad value by a running process is a GPU test
(tests/test_gpu_dropout_dev.py)."""
import ctypes as C
import re
from pathlib import Path

from graphaibench_amd import capi, layers as L

ROOT = Path(__file__).resolve().parent.parent
CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float}


def header_signature(name):
    """(restype, argtypes) of a prototype of include/gaib.h: every pointer is a void pointer in the table"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gaib.h").read_text(), flags=re.S)
    ret, args = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text).groups()
    types = []
    for a in args.split(","):
        a = a.strip()
        types.append(C.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
    return CTYPE[ret], types


def test_table_carries_the_header_signature():
    want = header_signature("gaib_dropout_dev")
    # ctx, n, scale, drop_rate, d_seed, d_in, d_masks, d_out
    assert want == (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    got = capi.SIGNATURES["gaib_dropout_dev"]
    assert got[0] is want[0] and list(got[1]) == want[1]
    # (the parser reads the by-value form as the table has it)
    by_value = capi.SIGNATURES["gaib_dropout"]
    assert (by_value[0], list(by_value[1])) == header_signature("gaib_dropout")
    assert callable(capi.Context.dropout_dev)


def test_null_context_is_an_error_without_a_gpu():
    lib = capi.load()
    assert hasattr(C.CDLL(str(capi.LIB_PATH)), "gaib_dropout_dev")
    assert lib.gaib_dropout_dev(None, 0, 1.0, 0.0, None, None, None, None) != 0
    assert b"gaib_dropout_dev" in lib.gaib_last_error() and b"NULL" in lib.gaib_last_error()
    assert lib.gaib_dropout_dev(None, 4, 2.0, 0.5, None, None, None, None) != 0


def test_seed_switch_parses():
    lib = L.load()
    assert lib.gaibl_parse_switch(b"0") == 0 and lib.gaibl_parse_switch(b"1") == 1
    for bad in (b"2", b"", b"10", b"yes", b"-1", b"1 ", None):
        assert lib.gaibl_parse_switch(bad) == -1, bad
    src = (ROOT / "graphaibench_amd" / "host" / "context.cpp").read_text()
    block = src[src.index('getenv("GAIB_DROP_SEED_DEV")'):]
    block = block[:block.index("gaib_set_option") + 60]
    assert "parse_switch(d)" in block and "expected 0 or 1" in block and '"drop_seed_dev"' in block
