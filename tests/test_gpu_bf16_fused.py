"""GPU suite, the fused aggregation + dense product over bf16 feature tables (gaib_spmm_gemm_bf16 / gaib_spmm_gemm2_bf16):
bit for bit against gaib_spmm_gemm(2) on the widened table over every route and kernel variant, the profile row of the fused
launch, the GCN / SAGE layers with agg_bf16 against the fp32 layers on representable inputs, the refusals, and a table that
is above 4 GB in fp32 and below in bf16."""
import numpy as np
import pytest
import torch

import test_gpu_bf16 as tb  # helpers of the plain bf16 suite (imported as a module: its tests are collected there, not here)
from graphaibench_amd import capi, layers as L
from test_gpu_bf16 import bf16_on, lctx  # noqa: F401  (fixtures)
from util import random_graph

pytestmark = pytest.mark.gpu
bits32 = tb.bits32

LEN_IN = [1, 16, 47, 64, 66, 100, 128, 130, 192, 256, 300]  # <= 64 | 65..128 | two K-slabs | not fusable
LEN_OUT = [16, 47, 128, 256]
KINDS = [capi.W_GCN, capi.W_MEAN, capi.W_MEAN_T, capi.W_EDGE]
FLAGS = [dict(), dict(relu=True), dict(agg_scratch=True), dict(accumulate=True)]


def graphs(ctx):
    for name, g, nc in tb.graphs(ctx):
        if name == "rect":  # (the fused call's layer shapes are square; rectangular column spaces are gaib_spmm_bf16's test)
            g.close()
            continue
        yield name, g, nc


class Tally:
    def __init__(self):
        self.compared = self.refused = 0


def compare(ctx, g, nc, len_in, len_out, kind, transW, flags, dual, gen, ew, tally):
    """spmm_gemm_bf16 on a random bf16 table against spmm_gemm on the widened table: the same bits, or refused alike"""
    nv = g.nv
    xb = torch.randn(nc, len_in, device="cuda", generator=gen).to(torch.bfloat16)
    xw = ctx.cast_bf16_f32(xb)
    wshape = (len_out, len_in) if transW else (len_in, len_out)
    W = torch.randn(wshape, device="cuda", generator=gen) * 0.2
    rows2 = torch.randn(nv, len_in, device="cuda", generator=gen) if dual else None
    W2 = torch.randn(wshape, device="cuda", generator=gen) * 0.2 if dual else None
    agg0 = torch.randn(nv, len_in, device="cuda", generator=gen)
    out0 = torch.randn(nv, len_out, device="cuda", generator=gen)
    w = ew if kind == capi.W_EDGE else None
    agg_r, agg_b, out_r, out_b = agg0.clone(), agg0.clone(), out0.clone(), out0.clone()
    kw = dict(transW=transW, edge_w=w, rows2=rows2, W2=W2, **flags)
    try:
        ctx.spmm_gemm(g, kind, xw, agg_r, W, out_r, **kw)
    except capi.GaibError:
        with pytest.raises(capi.GaibError):
            ctx.spmm_gemm_bf16(g, kind, xb, agg_b, W, out_b, **kw)
        tally.refused += 1
        return
    ctx.spmm_gemm_bf16(g, kind, xb, agg_b, W, out_b, **kw)
    what = (len_in, len_out, kind, transW, flags, dual)
    assert torch.equal(bits32(out_b), bits32(out_r)), ("out", what)
    if not flags.get("agg_scratch"):
        assert torch.equal(bits32(agg_b), bits32(agg_r)), ("agg", what)
    tally.compared += 1


def test_spmm_gemm_bf16_bit_identical(ctx):
    """1: every len_in class with every kind and both transW on every graph; len_out, flags and the second product rotate
    through the cross product (two picks per (len_in, kind, transW) on the two large graphs, one on the others)"""
    tally = Tally()
    gen = torch.Generator(device="cuda").manual_seed(11)
    for name, g, nc in graphs(ctx):
        full = name in ("random", "powerlaw_hub")
        lens = LEN_IN if full else [16, 64, 100, 128, 192, 300]
        ew = torch.rand(max(g.ne, 1), device="cuda", generator=gen) + 0.1
        k = 0
        for len_in in lens:
            for kind in KINDS:
                for transW in (0, 1):
                    for pick in range(2 if full else 1):
                        q = k + 5 * pick
                        compare(ctx, g, nc, len_in, LEN_OUT[q % 4], kind, bool(transW), FLAGS[(q // 4 + pick) % 4],
                                bool((q // 2 + pick) % 2), gen, ew, tally)
                    k += 1
        g.close()
    total = tally.compared + tally.refused
    print(f"compared {tally.compared}, refused alike {tally.refused}")
    assert tally.compared >= 420, tally.compared  # (2 x 176 + 2 x 48 = 448 argument sets)
    assert tally.refused <= 0.10 * total, (tally.refused, total)


# option -> value, with the options it needs next to it; every one selects a kernel variant or a route of the fp32 path
VARIANTS = [
    [("spmm_flat", 0)], [("spmm_flat", 1), ("spmm_flat_ring", 0)], [("spmm_flat", 1), ("spmm_flat_ring", 1)],
    [("spmm_tile_xcd", 0)], [("spmm_tile_xcd", 16)], [("spmm_tile_xcd", 1024), ("spmm_prefetch_ids", 1)],
    [("spmm_tile_xcd", 1024), ("spmm_prefetch_ids", 0)], [("spmm_addr_mode", 2)], [("spmm_addr_mode", 2), ("spmm_flat", 1)],
    [("spmm_fuse", 0)], [("spmm_chunked", 1)], [("spmm_pad", 0)], [("spmm_heavy_threshold", 64)],
    [("spmm_bf16_fuse_u", 16)], [("spmm_bf16_fuse_u", 32)],
]
DEFAULTS = dict(spmm_flat=-1, spmm_flat_ring=-1, spmm_tile_xcd=-1, spmm_prefetch_ids=1, spmm_addr_mode=0, spmm_fuse=1,
                spmm_chunked=-1, spmm_pad=1, spmm_heavy_threshold=1024, spmm_bf16_fuse_u=0)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "+".join(f"{k}={x}" for k, x in v))
def test_every_variant_gives_the_same_bits(ctx, variant):
    """2: the hub graph under each option that selects a kernel variant in the fp32 path"""
    rp, ci = random_graph(3000, 8, seed=2, power_law=True, hub_deg=2500)
    g = ctx.graph(rp, ci)
    gen = torch.Generator(device="cuda").manual_seed(13)
    ew = torch.rand(g.ne, device="cuda", generator=gen) + 0.1
    tally = Tally()
    try:
        for key, v in variant:
            ctx.set_option(key, v)
        k = 0
        for len_in in (16, 64, 100, 128, 256):
            for len_out in (47, 128):
                for kind in (capi.W_GCN, capi.W_MEAN):
                    compare(ctx, g, 3000, len_in, len_out, kind, bool(k % 3 == 0), FLAGS[k % 4], bool(k % 2), gen, ew, tally)
                    k += 1
    finally:
        for key, v in DEFAULTS.items():
            ctx.set_option(key, v)
        g.close()
    assert tally.compared == 20, (tally.compared, tally.refused)


def test_the_fused_kernel_is_what_ran(ctx):
    """3: 128 -> 128, W_GCN, default options: one fused launch over the bf16 table, no dense-product launch next to it"""
    n = 2000
    rp, ci = random_graph(n, 12, seed=1)
    g = ctx.graph(rp, ci)
    xb = torch.randn(n, 128, device="cuda").to(torch.bfloat16)
    W = torch.randn(128, 128, device="cuda")
    agg, out = torch.empty(n, 128, device="cuda"), torch.empty(n, 128, device="cuda")
    ctx.spmm_gemm_bf16(g, capi.W_GCN, xb, agg, W, out)  # (lazily built tables, workspace)
    torch.cuda.synchronize()
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        ctx.spmm_gemm_bf16(g, capi.W_GCN, xb, agg, W, out)
        torch.cuda.synchronize()
    finally:
        ctx.prof_enable(False)
    n_fused, _ = ctx.prof_get("spmm_gemm_bf16_fused")
    table = ctx.prof_table()
    ctx.prof_reset()
    g.close()
    assert n_fused >= 1, table
    others = [k for k in table if not k.startswith(("spmm_gemm_bf16_fused", "spmm_bf16_heavy"))]
    assert not others, others  # no sgemm row, no plain aggregation row


def round_bf16(a):
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize("selfloop", [True, False])
@pytest.mark.parametrize("arch", ["gcn", "sage"])
@pytest.mark.parametrize("din,dout,level", [(64, 128, 0), (128, 128, 1), (256, 256, 1)])
def test_layers_same_bits_on_representable_inputs(lctx, arch, selfloop, din, dout, level):
    """4: x and grad_in rounded to bf16 beforehand (the cast is exact), din <= dout (the gathered tables are x and grad_in
    themselves): the layer with bf16 tables computes what the fp32 layer computes, bit for bit"""
    rp, ci = tb.cora()
    n = 2708
    x, gin = round_bf16(tb.feat(n, din, 21)), round_bf16(tb.feat(n, dout, 22))
    kind = L.GCN if arch == "gcn" else L.SAGE
    res = {}
    try:
        for on in (1, 0):
            lctx.set_option("agg_bf16", on)
            g_d = L.LGraph.from_host(rp, ci, add_selfloop=selfloop)
            res[on] = tb.run_layer(kind, level, n, din, dout, g_d, x, gin)
            g_d.close()
    finally:
        lctx.set_option("agg_bf16", 0)
    keys = ["out", "Wg"] + (["Wsg"] if arch == "sage" else []) + (["go"] if level > 0 else [])
    for k in keys:
        a, b = res[1][k], res[0][k]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


@pytest.mark.parametrize("arch", ["gcn", "sage"])
@pytest.mark.parametrize("din,dout,level", [(128, 64, 1), (256, 256, 1), (256, 128, 0)])
def test_layers_within_the_bound_elsewhere(bf16_on, arch, din, dout, level):
    """4, the rest: unrounded inputs, and din > dout where the gathered table is a product -- the documented rounding bound
    (the check of the plain bf16 suite, on shapes that take the fused route and the K-slab route)"""
    tb.test_layers_with_bf16_tables(bf16_on, arch, din, dout, level)


def test_refusals(ctx):
    """5"""
    n = 500
    rp, ci = random_graph(n, 6, seed=4)
    g = ctx.graph(rp, ci)
    xb = torch.randn(n, 64, device="cuda").to(torch.bfloat16)
    xw = ctx.cast_bf16_f32(xb)
    W = torch.randn(64, 32, device="cuda")
    agg, out = torch.zeros(n, 64, device="cuda"), torch.zeros(n, 32, device="cuda")
    lib, h = ctx.lib, ctx.h
    p = lambda t: t.data_ptr() if t is not None else None

    def both(x32, x16, agg_t, W_t, out_t, rows2=None, W2=None, two=False, len_out=32, graph=g, flags=0):
        if two:
            r32 = lib.gaib_spmm_gemm2(h, graph.h, capi.W_MEAN, None, 64, p(x32), p(agg_t), p(W_t), 0, p(rows2), p(W2), len_out, p(out_t), flags)
            r16 = lib.gaib_spmm_gemm2_bf16(h, graph.h, capi.W_MEAN, None, 64, p(x16), p(agg_t), p(W_t), 0, p(rows2), p(W2), len_out, p(out_t), flags)
        else:
            r32 = lib.gaib_spmm_gemm(h, graph.h, capi.W_MEAN, None, 64, p(x32), p(agg_t), p(W_t), 0, len_out, p(out_t), flags)
            r16 = lib.gaib_spmm_gemm_bf16(h, graph.h, capi.W_MEAN, None, 64, p(x16), p(agg_t), p(W_t), 0, len_out, p(out_t), flags)
        return r32, r16

    # aliasing buffers (agg == out), rows2 without W2, an unknown flag: the fp32 call's code
    sq = torch.zeros(n, 64, device="cuda")
    for r32, r16 in (both(xw, xb, sq, torch.zeros(64, 64, device="cuda"), sq, len_out=64),
                     both(xw, xb, agg, W, out, rows2=torch.zeros(n, 64, device="cuda"), W2=None, two=True),
                     both(xw, xb, agg, W, out, flags=64)):
        assert r32 < 0 and r16 == r32, (r32, r16)
    # GAIB_OVERLAPS_TRANSFER belongs to partitioned runs: GAIB_ERR_INVALID
    assert lib.gaib_spmm_gemm_bf16(h, g.h, capi.W_MEAN, None, 64, p(xb), p(agg), p(W), 0, 32, p(out), 8) == -1
    assert b"OVERLAPS_TRANSFER" in lib.gaib_last_error()
    # len_out = 0 and a graph without rows: GAIB_OK, nothing written
    agg.fill_(3.0)
    out.fill_(5.0)
    assert both(xw, xb, agg, W, out, len_out=0) == (0, 0)
    g0 = ctx.graph(np.zeros(1, np.int64), np.zeros(0, np.uint32))
    assert both(xw, xb, agg, W, out, graph=g0) == (0, 0)
    g0.close()
    torch.cuda.synchronize()
    assert bool((agg == 3.0).all()) and bool((out == 5.0).all())
    # a graph with a row map (a row class of a partition): GAIB_ERR_UNSUPPORTED, with a message
    rmap = torch.arange(n, dtype=torch.int32, device="cuda")
    capi._check(lib.gaib_graph_set_row_map(h, g.h, rmap.data_ptr(), n), "gaib_graph_set_row_map")
    assert lib.gaib_spmm_gemm_bf16(h, g.h, capi.W_MEAN, None, 64, p(xb), p(agg), p(W), 0, 32, p(out), 0) == -5
    assert b"row map" in lib.gaib_last_error()
    rows2 = torch.zeros(n, 64, device="cuda")
    assert lib.gaib_spmm_gemm2_bf16(h, g.h, capi.W_MEAN, None, 64, p(xb), p(agg), p(W), 0, p(rows2), p(W), 32, p(out), 0) == -5
    g.close()


def test_table_above_4gb_as_fp32_below_as_bf16(ctx):
    """6: 9 M columns x 128: 2.3 GB in bf16 (buffer-descriptor gathers), 4.6 GB widened (64-bit addresses); columns at both
    ends of the table"""
    nv, nc, ln, lo = 320, 9_000_000, 128, 64
    assert nc * ln * 2 < 2 ** 32 < nc * ln * 4
    rng = np.random.default_rng(6)
    src = np.repeat(np.arange(nv), 12)
    dst = np.concatenate([rng.integers(0, 4096, nv * 4), rng.integers(0, nc, nv * 4), rng.integers(nc - 4096, nc, nv * 4)])
    g = ctx.graph(*tb.csr(nv, src, dst), ncols=nc)
    xb = torch.empty(nc, ln, dtype=torch.bfloat16, device="cuda")
    xb.normal_()
    xw = ctx.cast_bf16_f32(xb)
    ew = torch.rand(g.ne, device="cuda") + 0.1
    W = torch.randn(ln, lo, device="cuda") * 0.2
    try:
        for kind, w in ((capi.W_MEAN, None), (capi.W_EDGE, ew)):
            agg_r, agg_b = torch.empty(nv, ln, device="cuda"), torch.empty(nv, ln, device="cuda")
            out_r, out_b = torch.empty(nv, lo, device="cuda"), torch.empty(nv, lo, device="cuda")
            ctx.spmm_gemm(g, kind, xw, agg_r, W, out_r, edge_w=w)
            ctx.spmm_gemm_bf16(g, kind, xb, agg_b, W, out_b, edge_w=w)
            assert torch.equal(bits32(out_b), bits32(out_r)) and torch.equal(bits32(agg_b), bits32(agg_r)), kind
            assert float(out_r.abs().max()) > 0
    finally:
        del xw, xb
        g.close()
        torch.cuda.empty_cache()
