"""GPU suite, bf16 feature tables with a row stride (ld >= len): the strided cast against torch's CPU conversion and the dense
cast, gaib_spmm_bf16_ld / gaib_spmm_gemm_bf16_ld / gaib_spmm_gemm2_bf16_ld bit for bit against the dense calls on the same values
(the pad columns of every gathered table hold NaN bits: a pad value that reaches an output shows), the stride rule
gaib_bf16_row_stride, the refusals, the GCN / SAGE layers under spmm_bf16_pad = 1 against 0, and the profile rows."""
import numpy as np
import pytest
import torch

import test_gpu_bf16 as tb  # helpers of the plain bf16 suite (imported as a module: its tests are collected there, not here)
from graphaibench_amd import capi, layers as L
from test_gpu_bf16 import lctx  # noqa: F401  (fixture)
from util import random_graph

pytestmark = pytest.mark.gpu
bits32 = tb.bits32

N = 4000
PAIRS = [(1, 4), (17, 20), (47, 48), (47, 64), (100, 128), (128, 128), (200, 256)]  # (len, ld)
KINDS = [capi.W_GCN, capi.W_MEAN, capi.W_MEAN_T]
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
_HOST = {}


def host_graph(name):
    """(a) power law, ~20 edges per row, a hub row above the heavy threshold (1024); (b) short rows (the edge-stream forms);
    (c) a dense one (run with spmm_chunked = 1); (sparse) ne <= 4 nc, for the rule"""
    if name not in _HOST:
        if name == "a":
            _HOST[name] = random_graph(N, 20, seed=31, power_law=True, hub_deg=1500)
        elif name == "b":
            _HOST[name] = random_graph(N, 5, seed=32)
        elif name == "c":
            _HOST[name] = random_graph(N, 64, seed=33)
        else:
            _HOST[name] = random_graph(N, 3, seed=34)
    return _HOST[name]


def bits16(t):
    return t.contiguous().view(torch.int16)


def strided(xb, ld):
    """the [n x ld] table whose first columns are xb and whose pad columns hold NaN bits"""
    n, ln = xb.shape
    t = torch.full((n, ld), -1, dtype=torch.int16, device=xb.device)  # 0xffff: a NaN
    t[:, :ln] = bits16(xb)
    return t.view(torch.bfloat16)


# ---- 1: the strided cast ------------------------------------------------------------------------------------------------
# -0.0 and +0.0, -inf and +inf, a negative and a positive subnormal, a value that rounds up into the next exponent (-> 0x4000)
# and the largest finite float (rounds up to +inf): the words every cast below must be fed
KEY = np.array([0x80000000, 0x00000000, 0xff800000, 0x7f800000, 0x80000001, 0x007fffff, 0x3fffffff, 0x7f7fffff], np.uint32)
KEY_BF16 = np.array([0x8000, 0x0000, 0xff80, 0x7f80, 0x8000, 0x0080, 0x4000, 0x7f80], np.uint16)


def cast_words(rows, ln, rng):
    """random words with the special ones written inside the window: rows 0, rows / 2 and rows - 1 start with the special
    patterns (each row at another offset, so that they meet every lane of a group) and end with KEY, -0.0 in column
    len - 1: the last 8-element group of a row, which straddles len where len % 8 != 0"""
    e = np.arange(256, dtype=np.uint32) << 23  # every exponent around the rounding point: round-ups into the next exponent
    pat = np.concatenate([KEY, np.array(tb.SPECIAL, np.uint32), e | 0x7f8000, e | 0x7fffff | 0x80000000, e | 0x8000])
    words = rng.integers(0, 2 ** 32, (rows, ln), dtype=np.uint32)
    k = min(len(KEY), ln // 2)
    for j, r in enumerate(sorted({0, rows // 2, rows - 1})):
        words[r] = np.resize(np.roll(pat, -3 * j), ln)
        if k:
            words[r, ln - k:] = KEY[:k][::-1]
    return words


def check_cast(ctx, words, ld):
    rows, ln = words.shape
    f = words.view(np.float32)
    x = torch.from_numpy(f).cuda()
    buf = torch.full((rows * ld + 64,), 0x1234, dtype=torch.int16, device="cuda")  # a canary behind the last row
    out = buf[:rows * ld].view(torch.bfloat16).view(rows, ld)
    ctx.cast_f32_bf16_rows(x, ld, out)
    got = bits16(out).cpu().numpy().view(np.uint16)
    assert bool((buf[rows * ld:] == 0x1234).all()), (ln, ld)
    want = torch.from_numpy(f).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(f)
    assert np.array_equal(got[:, :ln][~nan], want[~nan]), (ln, ld)
    assert not got[:, ln:].any(), (ln, ld)  # +0.0 bits
    dense = bits16(ctx.cast_f32_bf16(x)).cpu().numpy().view(np.uint16)  # NaNs included: the dense cast's bits
    assert np.array_equal(got[:, :ln], dense), (ln, ld)
    for kw, kb in zip(KEY, KEY_BF16):  # (not through `want`: the bits themselves, the sign of a zero included)
        assert np.array_equal(got[:, :ln][words == kw], np.full(int((words == kw).sum()), kb, np.uint16)), (ln, ld, hex(kw))
    return x, out, dense


@pytest.mark.parametrize("rows", [1, 257, 4001])
def test_cast_rows(ctx, rows):
    rng = np.random.default_rng(rows)
    for ln, ld in PAIRS:
        words = cast_words(rows, ln, rng)
        if ln // 2 < len(KEY):  # rows too narrow to hold them (one column): one table per special word, in every row
            for kw in KEY:
                check_cast(ctx, np.full((rows, ln), kw, np.uint32), ld)
        else:
            for kw in KEY:
                assert (words == kw).any(), (ln, ld, hex(kw))
            assert words[rows - 1, ln - 1] == 0x80000000  # -0.0 next to the pad columns
        x, out, dense = check_cast(ctx, words, ld)
        if rows == 257:  # ld == len through the strided entry point, and a misaligned output (the element-wise form)
            same = bits16(ctx.cast_f32_bf16_rows(x, ln)).cpu().numpy().view(np.uint16)
            assert np.array_equal(same, dense), ln
            buf2 = torch.full((rows * ld + 65,), 0x1234, dtype=torch.int16, device="cuda")
            out2 = buf2[1:rows * ld + 1].view(torch.bfloat16).view(rows, ld)
            capi._check(ctx.lib.gaib_cast_f32_bf16_rows(ctx.h, rows, ln, x.data_ptr(), ld, out2.data_ptr()), "cast rows")
            assert torch.equal(bits16(out2), bits16(out)) and int(buf2[0]) == 0x1234 and bool((buf2[rows * ld + 1:] == 0x1234).all())
            # a misaligned input (one float off a 16-B boundary) under an aligned output: the 16-B stores with float-by-float
            # loads at a len % 4 == 0 too
            xoff = torch.empty(rows * ln + 1, device="cuda")[1:].view(rows, ln)
            xoff.copy_(x)
            assert x.data_ptr() % 16 == 0 and xoff.data_ptr() % 16 == 4
            buf3 = torch.full((rows * ld + 64,), 0x1234, dtype=torch.int16, device="cuda")
            capi._check(ctx.lib.gaib_cast_f32_bf16_rows(ctx.h, rows, ln, xoff.data_ptr(), ld, buf3.data_ptr()), "cast rows")
            assert torch.equal(buf3[:rows * ld].view(rows, ld), bits16(out)) and bool((buf3[rows * ld:] == 0x1234).all()), (ln, ld)


# ---- 2: plain aggregation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 4, 8])
@pytest.mark.parametrize("gname", ["a", "b", "c"])
def test_spmm_bf16_ld_bit_identical(ctx, gname, layout):
    g = ctx.graph(*host_graph(gname))
    gen = torch.Generator(device="cuda").manual_seed(41)
    n_checked = 0
    try:
        ctx.set_option("spmm_bf16_layout", layout)
        if gname == "c":
            ctx.set_option("spmm_chunked", 1)
        for ln, ld in PAIRS + [(300, 304), (128, 132)]:  # (128, 132): a len % 8 == 0 at an ld % 8 == 4
            xb = torch.randn(N, ln, device="cuda", generator=gen).to(torch.bfloat16)
            xs = strided(xb, ld)
            for kind in KINDS:
                for acc, relu in ((False, False), (True, False), (False, True)):
                    init = torch.randn(N, ln, device="cuda", generator=gen)
                    ref, got = init.clone(), init.clone()
                    ctx.spmm_bf16(g, kind, xb, ref, accumulate=acc, relu=relu)
                    ctx.spmm_bf16(g, kind, xs, got, accumulate=acc, relu=relu, ld=ld)
                    assert torch.equal(bits32(got), bits32(ref)), (gname, layout, ln, ld, kind, acc, relu)
                    assert not bool(torch.isnan(got).any())
                    n_checked += 1
    finally:
        ctx.set_option("spmm_bf16_layout", 0)
        ctx.set_option("spmm_chunked", -1)
        g.close()
    assert n_checked == 81


# ---- 3: fused -----------------------------------------------------------------------------------------------------------
FUSED_SHAPES = [(47, 128, 64), (100, 128, 128), (128, 47, 128), (200, 64, 256), (64, 64, 64)]  # (len_in, len_out, ld)
FUSED_FLAGS = [dict(), dict(agg_scratch=True), dict(relu=True, transW=True), dict(accumulate=True), dict(dual=True),
               dict(dual=True, relu=True, transW=True, agg_scratch=True)]


def fused_pair(ctx, g, kind, len_in, len_out, ld, gen, transW=False, dual=False, **flags):
    xb = torch.randn(N, len_in, device="cuda", generator=gen).to(torch.bfloat16)
    xs = strided(xb, ld)
    wshape = (len_out, len_in) if transW else (len_in, len_out)
    W = torch.randn(wshape, device="cuda", generator=gen) * 0.2
    rows2 = torch.randn(N, len_in, device="cuda", generator=gen) if dual else None
    W2 = torch.randn(wshape, device="cuda", generator=gen) * 0.2 if dual else None
    agg0 = torch.randn(N, len_in, device="cuda", generator=gen)
    out0 = torch.randn(N, len_out, device="cuda", generator=gen)
    agg_r, agg_s, out_r, out_s = agg0.clone(), agg0.clone(), out0.clone(), out0.clone()
    kw = dict(transW=transW, rows2=rows2, W2=W2, **flags)
    ctx.spmm_gemm_bf16(g, kind, xb, agg_r, W, out_r, **kw)
    ctx.spmm_gemm_bf16(g, kind, xs, agg_s, W, out_s, ld=ld, **kw)
    what = (len_in, len_out, ld, kind, transW, dual, flags)
    assert torch.equal(bits32(out_s), bits32(out_r)), ("out", what)
    assert not bool(torch.isnan(out_s).any()), what
    if not flags.get("agg_scratch"):
        assert torch.equal(bits32(agg_s), bits32(agg_r)), ("agg", what)


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("gname", ["a", "b"])
def test_spmm_gemm_bf16_ld_bit_identical(ctx, gname, fuse):
    """graph a: the row forms, the heavy row, two products, the K-slabs (200 columns); graph b: the edge-stream forms;
    spmm_fuse = 0: the two-kernel route"""
    g = ctx.graph(*host_graph(gname))
    gen = torch.Generator(device="cuda").manual_seed(43)
    try:
        ctx.set_option("spmm_fuse", fuse)
        for ring in ((1, 0) if gname == "b" and fuse else (1,)):
            ctx.set_option("spmm_flat_ring", ring)
            k = 0
            for len_in, len_out, ld in FUSED_SHAPES:
                for fl in FUSED_FLAGS:
                    fused_pair(ctx, g, (capi.W_GCN, capi.W_MEAN, capi.W_MEAN_T)[k % 3], len_in, len_out, ld, gen, **fl)
                    k += 1
    finally:
        ctx.set_option("spmm_fuse", 1)
        ctx.set_option("spmm_flat_ring", -1)
        g.close()


# ---- 4: 64-bit addressing -----------------------------------------------------------------------------------------------
def test_global_load_path(ctx):
    """spmm_addr_mode = 2 (the means of test_gpu_bf16_fused.py): global loads instead of the buffer descriptor"""
    gen = torch.Generator(device="cuda").manual_seed(45)
    try:
        ctx.set_option("spmm_addr_mode", 2)
        for gname in ("a", "b"):
            g = ctx.graph(*host_graph(gname))
            xb = torch.randn(N, 47, device="cuda", generator=gen).to(torch.bfloat16)
            ref, got = torch.empty(N, 47, device="cuda"), torch.empty(N, 47, device="cuda")
            ctx.spmm_bf16(g, capi.W_GCN, xb, ref)
            ctx.spmm_bf16(g, capi.W_GCN, strided(xb, 64), got, ld=64)
            assert torch.equal(bits32(got), bits32(ref)), gname
            fused_pair(ctx, g, capi.W_GCN, 47, 128, 64, gen)
            fused_pair(ctx, g, capi.W_MEAN, 47, 128, 64, gen, dual=True)
            g.close()
    finally:
        ctx.set_option("spmm_addr_mode", 0)


# ---- 5: the rule and the refusals --------------------------------------------------------------------------------------
def test_row_stride_rule(ctx):
    ga, gs = ctx.graph(*host_graph("a")), ctx.graph(*host_graph("sparse"))
    try:
        assert ga.ne > 4 * N >= gs.ne
        assert [ctx.bf16_row_stride(ga, ln) for ln in (47, 100, 128, 200)] == [64, 128, 128, 200]
        assert [ctx.bf16_row_stride(ga, ln) for ln in (1, 16, 64, 256)] == [1, 16, 64, 256]
        assert [ctx.bf16_row_stride(gs, ln) for ln in (47, 100, 128, 200)] == [47, 100, 128, 200]
        ctx.set_option("spmm_bf16_pad", 0)
        assert [ctx.bf16_row_stride(ga, ln) for ln in (47, 100, 128, 200)] == [47, 100, 128, 200]
        ctx.set_option("spmm_bf16_pad", 1)
        rmap = torch.arange(N, dtype=torch.int32, device="cuda")
        capi._check(ctx.lib.gaib_graph_set_row_map(ctx.h, ga.h, rmap.data_ptr(), N), "gaib_graph_set_row_map")
        assert ctx.bf16_row_stride(ga, 47) == 47
    finally:
        ctx.set_option("spmm_bf16_pad", 1)
        ga.close()
        gs.close()


def test_refusals(ctx):
    g = ctx.graph(*host_graph("a"))
    lib, h = ctx.lib, ctx.h
    x = torch.zeros(N, 64, dtype=torch.bfloat16, device="cuda")
    W = torch.zeros(47, 32, device="cuda")
    rows2 = torch.zeros(N, 47, device="cuda")
    out = torch.full((N, 47), 7.0, device="cuda")
    agg = torch.full((N, 47), 3.0, device="cuda")
    y = torch.full((N, 32), 5.0, device="cuda")
    p = lambda t: t.data_ptr()

    def two(ld, flags=0):
        return (lib.gaib_spmm_gemm_bf16_ld(h, g.h, capi.W_MEAN, None, 47, ld, p(x), p(agg), p(W), 0, 32, p(y), flags),
                lib.gaib_spmm_gemm2_bf16_ld(h, g.h, capi.W_MEAN, None, 47, ld, p(x), p(agg), p(W), 0, p(rows2), p(W), 32, p(y), flags))

    def three(ld):
        return (lib.gaib_spmm_bf16_ld(h, g.h, capi.W_MEAN, None, 47, ld, p(x), p(out), 0),) + two(ld)

    try:
        assert three(46) == (ERR_INVALID,) * 3  # ld < len
        assert b"ld" in lib.gaib_last_error()
        assert three(50) == (ERR_INVALID,) * 3  # ld != len and ld % 4 != 0
        assert three(63) == (ERR_INVALID,) * 3
        assert two(64, flags=8) == (ERR_INVALID,) * 2  # GAIB_OVERLAPS_TRANSFER
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((agg == 3.0).all()) and bool((y == 5.0).all())
        rmap = torch.arange(N, dtype=torch.int32, device="cuda")
        capi._check(lib.gaib_graph_set_row_map(h, g.h, rmap.data_ptr(), N), "gaib_graph_set_row_map")
        assert three(64) == (ERR_UNSUPPORTED,) * 3
        assert b"row map" in lib.gaib_last_error()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((agg == 3.0).all()) and bool((y == 5.0).all())
    finally:
        g.close()


# ---- 6: the layers ---------------------------------------------------------------------------------------------------------
def run_layer(lctx, kind, n, din, dout, g_d, x, gin):
    """a level-1 layer, forward + backward; the stride of the table the forward pass cast (agg_bf16_ld_last) next to the results"""
    ld = L.Layer(kind, 1, n, din, dout, g_d, False)
    ld.write(L.FEAT_IN, tb.dev(x))
    out = torch.empty(n, dout, device="cuda")
    ld.forward(out)
    ld_fwd = lctx.get_option("agg_bf16_ld_last")
    ld.write(L.GRAD_IN, tb.dev(gin))
    grad_out = torch.zeros(n, din, device="cuda")
    ld.backward(out, grad_out)
    L.sync()
    res = dict(out=out.cpu().numpy(), go=grad_out.cpu().numpy(), Wg=ld.tensor(L.W_NEIGH_GRAD, (din, dout)).cpu().numpy())
    if kind == L.SAGE:
        res["Wsg"] = ld.tensor(L.W_SELF_GRAD, (din, dout)).cpu().numpy()
    ld.close()
    return res, ld_fwd, lctx.get_option("agg_bf16_ld_last")


@pytest.mark.parametrize("arch", ["gcn", "sage"])
@pytest.mark.parametrize("din,dout", [(128, 47), (100, 128)])
def test_layers_padded_against_dense_stride(lctx, arch, din, dout):
    """either pass aggregates at the narrower of the two widths: forward the product (47 columns) or the input (100), backward
    the gradient (47) or its product with W^T (100)"""
    rp, ci = host_graph("a")
    x, gin = tb.feat(N, din, 51), tb.feat(N, dout, 52)
    kind = L.GCN if arch == "gcn" else L.SAGE
    narrow = min(din, dout)
    padded = {47: 64, 100: 128}
    res = {}
    try:
        for bf in (1, 0):
            for pad in (1, 0):
                lctx.set_option("agg_bf16", bf)
                lctx.set_option("spmm_bf16_pad", pad)
                lctx.set_option("agg_bf16_ld_last", 0)
                g_d = L.LGraph.from_host(rp, ci, add_selfloop=arch == "gcn")
                res[bf, pad], ld_fwd, ld_bwd = run_layer(lctx, kind, N, din, dout, g_d, x, gin)
                g_d.close()
                if bf:
                    assert ld_fwd == (padded[narrow] if pad else narrow), (pad, ld_fwd)
                    assert ld_bwd == (padded[narrow] if pad else narrow), (pad, ld_bwd)
                else:
                    assert ld_fwd == 0 and ld_bwd == 0  # no table was cast
    finally:
        lctx.set_option("agg_bf16", 0)
        lctx.set_option("spmm_bf16_pad", 1)
    for bf in (1, 0):
        for k, a in res[bf, 1].items():
            b = res[bf, 0][k]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (bf, k, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
    assert not np.array_equal(res[1, 1]["out"], res[0, 1]["out"])  # (the bf16 tables were in use)


# ---- 7: the profile ------------------------------------------------------------------------------------------------------
def test_profile_rows_of_a_strided_call(ctx):
    """the same keys, counts, algorithmic bytes (2 len per gathered row, not 2 ld) and flops as the dense call"""
    g = ctx.graph(*host_graph("a"))
    gen = torch.Generator(device="cuda").manual_seed(47)
    W = torch.randn(100, 128, device="cuda", generator=gen)
    x47 = torch.randn(N, 47, device="cuda", generator=gen).to(torch.bfloat16)
    x100 = torch.randn(N, 100, device="cuda", generator=gen).to(torch.bfloat16)
    s47, s100 = strided(x47, 64), strided(x100, 128)
    out, agg, y = torch.empty(N, 47, device="cuda"), torch.empty(N, 100, device="cuda"), torch.empty(N, 128, device="cuda")

    def dense():
        ctx.spmm_bf16(g, capi.W_GCN, x47, out)
        ctx.spmm_gemm_bf16(g, capi.W_GCN, x100, agg, W, y)

    def padded():
        ctx.spmm_bf16(g, capi.W_GCN, s47, out, ld=64)
        ctx.spmm_gemm_bf16(g, capi.W_GCN, s100, agg, W, y, ld=128)

    tabs = []
    try:
        for fn in (dense, padded):
            fn()  # (lazily built tables, workspace)
            torch.cuda.synchronize()
            ctx.prof_reset()
            ctx.prof_enable(True)
            fn()
            torch.cuda.synchronize()
            ctx.prof_enable(False)
            tabs.append(ctx.prof_table())
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
        g.close()
    d, s = tabs
    assert set(d) == set(s), (sorted(d), sorted(s))
    assert {"spmm_bf16_light", "spmm_bf16_heavy", "spmm_gemm_bf16_fused"} <= {k.split("@")[0] for k in d}, sorted(d)
    for k in d:
        assert (d[k]["count"], d[k]["bytes"], d[k]["flops"]) == (s[k]["count"], s[k]["bytes"], s[k]["flops"]), (k, d[k], s[k])
