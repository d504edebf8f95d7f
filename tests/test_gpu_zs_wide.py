"""GPU suite, wide zero-suppressed tables (256 columns: one packed image per 128-column K-slab).  gaib_pack_zs_wide against
gaib_pack_zs on the two column halves and the round trip bit for bit; the packed K-slab aggregation (gaib_spmm_gemm_zs /
gaib_spmm_gemm2_zs at len_in = 256) bit for bit against gaib_spmm_gemm(2) on the dense table; the refusals; the GCN / SAGE
256 -> 256 layers with agg_zs_wide 1 against 0; the guard counted in row-slabs; the trainer's switch.
A half row (128 columns of one slab) holds 46 values per parity: 46 + 46 fit, 47 in one parity never does."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from graphaibench_amd import capi, layers as L
from test_gpu_bf16 import make_dataset
from test_gpu_zs import CAP, bits32, graphs, pack_reference, row_with
from util import random_graph

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SPECIALS = np.array([0x80000000, 0x7fc00000, 0xffc00001, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x7fffffff], np.uint32)


# ---- the pack -----------------------------------------------------------------------------------------------------------
def fixed_rows(rng) -> np.ndarray:
    """[4 x 256] bit patterns: 46 + 46 values in slab 1 and none in slab 0 (fits); 47 in the even half of slab 0 only; 47 in the
    odd half of slab 1 only; -0.0, NaN, +-inf and subnormals among values and zeros"""
    t = np.zeros((4, 256), np.uint32)
    t[0, 128:] = row_with(2 * CAP, rng, n_even=CAP)
    t[1, :128] = row_with(CAP + 1 + 20, rng, n_even=CAP + 1)
    t[1, 128:] = row_with(40, rng)
    t[2, :128] = row_with(40, rng)
    t[2, 128:] = row_with(CAP + 1 + 20, rng, n_even=20)
    t[3, :128] = row_with(50, rng)
    t[3, 128:] = row_with(50, rng)
    t[3, [1, 2, 5, 70, 127, 128, 129, 200, 254, 255]] = np.resize(SPECIALS, 10)
    return t


def wide_table(rows: int, kept: float, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = rng.integers(1, 2 ** 32, (rows, 256), dtype=np.uint32)
    t[rng.random((rows, 256)) >= kept] = 0
    if rows >= 4:
        t[:4] = fixed_rows(rng)
    return t


def check_pack(ctx, t: np.ndarray):
    rows = t.shape[0]
    x = torch.from_numpy(t.view(np.int32)).cuda().view(torch.float32)
    over = torch.zeros(1, dtype=torch.int32, device="cuda")
    zs = ctx.pack_zs_wide(x, overflow=over)
    assert tuple(zs.shape) == (2, rows, 96)
    n_over = 0
    for s in range(2):
        half = x[:, 128 * s:128 * s + 128].contiguous()
        o = torch.zeros(1, dtype=torch.int32, device="cuda")
        want = ctx.pack_zs(half, overflow=o)
        assert torch.equal(zs[s], want), (s, torch.nonzero(zs[s] != want)[:10])
        if rows <= 5:  # ... and so both equal the format restated
            assert np.array_equal(zs[s].cpu().numpy().view(np.uint32), pack_reference(t[:, 128 * s:128 * s + 128]))
        n_over += int(o.item())
    assert int(over.item()) == n_over  # row-slabs: a row over capacity in both halves counts twice
    ne, no = (t[:, 0::2] != 0), (t[:, 1::2] != 0)
    by_hand = sum(int(((ne[:, 64 * s:64 * s + 64].sum(axis=1) > CAP) | (no[:, 64 * s:64 * s + 64].sum(axis=1) > CAP)).sum()) for s in range(2))
    assert n_over == by_hand
    back = ctx.unpack_zs_wide(zs, x)
    assert torch.equal(bits32(back), bits32(x))
    return zs.cpu().numpy().view(np.uint32), n_over


@pytest.mark.parametrize("kept", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("rows", [1, 4, 5, 1000])
def test_pack_wide_is_two_narrow_packs_and_round_trips(ctx, rows, kept):
    got, n_over = check_pack(ctx, wide_table(rows, kept, seed=rows))
    if rows >= 4:
        # the fixed rows: 46 + 46 in slab 1 is packed, 47 in one half keeps its masks only -- in that slab alone
        assert np.count_nonzero(got[1, 0, 4:]) == 2 * CAP and np.count_nonzero(got[0, 0]) == 0
        assert np.count_nonzero(got[0, 1, 4:]) == 0 and np.count_nonzero(got[1, 1, 4:]) == 40
        assert np.count_nonzero(got[0, 2, 4:]) == 40 and np.count_nonzero(got[1, 2, 4:]) == 0
        assert n_over >= 2
    if kept == 1.0 and rows == 1000:
        assert n_over == 2 * (rows - 4) + 2  # every row twice, but for the fixed ones


def test_pack_wide_single_rows(ctx):
    """each fixed row as a table of one row (the last wave of the grid alone, slab 1 right behind slab 0's only row)"""
    f = fixed_rows(np.random.default_rng(77))
    for r in range(4):
        _, n_over = check_pack(ctx, f[r:r + 1].copy())
        assert n_over == (0, 1, 1, 0)[r]


def test_pack_wide_refuses_other_widths(ctx):
    for ln in (128, 192, 384):
        x = torch.ones(8, ln, device="cuda")
        out = torch.full((2 * 8 * 96,), 7, dtype=torch.int32, device="cuda")
        over = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = ctx.lib.gaib_pack_zs_wide(ctx.h, 8, ln, x.data_ptr(), out.data_ptr(), over.data_ptr())
        assert rc == -5, (ln, rc)
        dense = torch.full((8, ln), 3.0, device="cuda")
        rc = ctx.lib.gaib_unpack_zs_wide(ctx.h, 8, ln, out.data_ptr(), x.data_ptr(), dense.data_ptr())
        assert rc == -5, (ln, rc)
        torch.cuda.synchronize()
        assert bool((out == 7).all()) and int(over.item()) == 0 and bool((dense == 3.0).all())


# ---- the packed K-slab aggregation --------------------------------------------------------------------------------------
def half_over(x):
    """[rows x 2] bool: is the half row of slab s over capacity?"""
    nz = bits32(x) != 0
    ev, od = nz[:, 0::2], nz[:, 1::2]
    return torch.stack([(ev[:, 64 * s:64 * s + 64].sum(dim=1) > CAP) | (od[:, 64 * s:64 * s + 64].sum(dim=1) > CAP) for s in range(2)], dim=1)


def masked_table(n, density, gen, over_mix=False):
    """normal values, a share `density` of them kept (the rest +0.0).  over_mix: every fifth row dense in both slabs, every seventh
    over capacity in slab 1 only, every eleventh in slab 0 only (93 values in that half row: 47 even columns)"""
    def draw(rows, cols, keep):
        v = torch.randn(rows, cols, device="cuda", generator=gen)
        if keep <= 0.0:
            v.zero_()
        elif keep < 1.0:
            v = v * (torch.rand(rows, cols, device="cuda", generator=gen) < keep)
        return torch.where(v == 0, torch.zeros_like(v), v)  # (no -0.0 from the product)

    x = draw(n, 256, density)
    if over_mix:
        idx = torch.arange(n, device="cuda")
        r5, r7, r11 = idx[0::5], idx[3::7], idx[5::11]
        r7 = r7[r7 % 5 != 0]
        r11 = r11[(r11 % 5 != 0) & (r11 % 7 != 3)]
        x[r5] = draw(len(r5), 256, 1.0)
        for rr, s in ((r7, 1), (r11, 0)):
            blk = draw(len(rr), 256, 0.25)
            blk[:, 128 * s:128 * s + 93] = draw(len(rr), 93, 1.0)
            blk[:, 128 * s + 93:128 * s + 128] = 0.0
            x[rr] = blk
    return x.contiguous()


def compare(ctx, g, x, kind, len_out, transW, flags, dual, gen, ew=None):
    nv = g.nv
    zs = ctx.pack_zs_wide(x)
    wshape = (len_out, 256) if transW else (256, len_out)
    W = torch.randn(wshape, device="cuda", generator=gen) * 0.2
    rows2 = torch.randn(nv, 256, device="cuda", generator=gen) if dual else None
    W2 = torch.randn(wshape, device="cuda", generator=gen) * 0.2 if dual else None
    agg0 = torch.randn(nv, 256, device="cuda", generator=gen)
    out0 = torch.randn(nv, len_out, device="cuda", generator=gen)
    agg_r, agg_z, out_r, out_z = agg0.clone(), agg0.clone(), out0.clone(), out0.clone()
    kw = dict(transW=transW, rows2=rows2, W2=W2, edge_w=ew if kind == capi.W_EDGE else None, **flags)
    ctx.spmm_gemm(g, kind, x, agg_r, W, out_r, **kw)
    assert ctx.spmm_gemm_zs(g, kind, x, zs, agg_z, W, out_z, **kw), "refused"
    what = (kind, len_out, transW, flags, dual)
    assert torch.equal(bits32(out_z), bits32(out_r)), ("out", what)
    if flags.get("agg_scratch"):
        assert torch.equal(bits32(agg_z), bits32(agg0)), ("scratch agg touched", what)
    else:
        assert torch.equal(bits32(agg_z), bits32(agg_r)), ("agg", what)


FLAGS = [dict(), dict(relu=True), dict(agg_scratch=True), dict(accumulate=True), dict(relu=True, agg_scratch=True)]
LEN_OUT = (256, 128, 16)  # the 2-row strip (a [256 x 128] slab of op(W) fills LDS) and the 8-row strip


def test_spmm_gemm_zs_wide_bit_identical(ctx):
    """every graph x density x weight kind x one / two products; transW, the flags and len_out are drawn independently (seeded);
    the call the layers' backward makes -- transW, the aggregate as scratch, 256 outputs -- runs on every graph and density with
    one and with two products"""
    gen = torch.Generator(device="cuda").manual_seed(5)
    rng = np.random.default_rng(17)
    n = 0
    seen, seen_out = set(), set()
    for name, g, nc in graphs(ctx):
        assert g.ne >= 12 * g.nv or name == "single_vertex", (name, g.ne, g.nv)
        if name == "single_vertex":  # one edge: the dense call streams edges on its first slab unless told not to
            ctx.set_option("spmm_flat", 0)
        try:
            ew = torch.rand(max(g.ne, 1), device="cuda", generator=gen) + 0.1
            for density in (0.0, 0.25, 0.5, 0.75, 1.0, "mix"):
                x = masked_table(nc, 0.5 if density == "mix" else density, gen, over_mix=density == "mix")
                if density == "mix" and nc >= 100:
                    ho = half_over(x)
                    both, only1, only0 = ho[:, 0] & ho[:, 1], ~ho[:, 0] & ho[:, 1], ho[:, 0] & ~ho[:, 1]
                    assert int(both.sum()) >= nc // 5 and int(only1.sum()) >= nc // 10 and int(only0.sum()) >= nc // 20
                    assert int((~ho[:, 0] & ~ho[:, 1]).sum()) >= nc // 2
                compare(ctx, g, x, capi.W_GCN, 256, True, dict(agg_scratch=True), False, gen, ew)
                compare(ctx, g, x, capi.W_MEAN_T, 256, True, dict(agg_scratch=True), True, gen, ew)
                for kind in (capi.W_GCN, capi.W_MEAN_T, capi.W_MEAN, capi.W_EDGE):
                    for dual in (False, True):
                        transW, fl, len_out = bool(rng.integers(2)), int(rng.integers(len(FLAGS))), LEN_OUT[int(rng.integers(3))]
                        compare(ctx, g, x, kind, len_out, transW, FLAGS[fl], dual, gen, ew)
                        seen.add((dual, transW, fl))
                        seen_out.add((len_out, dual, kind in (capi.W_MEAN,)))
                        n += 1
        finally:
            ctx.set_option("spmm_flat", -1)
        g.close()
    assert n == 4 * 6 * 4 * 2
    assert len(seen) == 2 * 2 * len(FLAGS), sorted(seen)  # every (products, transW, flags) combination was drawn
    # every width (both strips) with one and two products, with per-row (MEAN) and per-edge weights
    assert len(seen_out) == 3 * 2 * 2, sorted(seen_out)


def test_special_values_aggregate_alike(ctx):
    """-0.0, inf and NaN in both slabs: stored, gathered and multiplied like any value (NaN payloads are the hardware's on both sides)"""
    gen = torch.Generator(device="cuda").manual_seed(9)
    rp, ci = random_graph(500, 30, seed=4)
    g = ctx.graph(rp, ci)
    x = masked_table(500, 0.5, gen)
    x[::7, 3] = -0.0
    x[::11, 64] = float("inf")
    x[::13, 127] = float("nan")
    x[::5, 128] = float("-inf")
    x[::9, 200] = -0.0
    x[::17, 255] = float("nan")
    for len_out in (256, 128):
        compare(ctx, g, x, capi.W_GCN, len_out, True, dict(), False, gen)
    g.close()


def test_refusals(ctx):
    gen = torch.Generator(device="cuda").manual_seed(6)
    n = 600
    rp, ci = random_graph(n, 30, seed=7)
    g = ctx.graph(rp, ci)
    assert g.ne >= 12 * g.nv
    x = masked_table(n, 0.5, gen)
    zs = ctx.pack_zs_wide(x)
    W = torch.randn(256, 256, device="cuda", generator=gen) * 0.1
    agg, out = torch.full((n, 256), 7.0, device="cuda"), torch.full((n, 256), 7.0, device="cuda")
    p = lambda t: t.data_ptr()

    def refused(g_, x_, zs_, agg_, W_, len_in, what):
        assert ctx.lib.gaib_spmm_gemm_zs_route(ctx.h, g_.h, capi.W_GCN, len_in, p(x_), p(zs_), p(agg_), None, 256, p(out)) == -5, what
        assert ctx.spmm_gemm_zs(g_, capi.W_GCN, x_, zs_, agg_, W_, out) is False, what
        assert ctx.spmm_gemm_zs(g_, capi.W_MEAN_T, x_, zs_, agg_, W_, out, rows2=x_, W2=W_) is False, what
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((agg_ == 7.0).all()), what  # nothing was launched

    # 64-bit addressing, the two-kernel route, the ordered chunks, the edge stream, the XCD-affine tile supply
    for key, v, back in (("spmm_addr_mode", 2, 0), ("spmm_fuse", 0, 1), ("spmm_chunked", 1, -1), ("spmm_flat", 1, -1),
                         ("spmm_tile_xcd", 1024, -1)):
        ctx.set_option(key, v)
        try:
            refused(g, x, zs, agg, W, 256, key)
        finally:
            ctx.set_option(key, back)
    # an image off its 128-B boundary
    buf = torch.empty(2 * n * 96 + 8, dtype=torch.int32, device="cuda")
    refused(g, x, buf[8:].view(2, n, 96), agg, W, 256, "alignment")
    # a width between the two: a second slab narrower than 128 columns has no packed form (whatever image comes with it)
    x200 = masked_table(n, 0.5, gen)[:, :200].contiguous()
    a200, W200 = torch.full((n, 200), 7.0, device="cuda"), torch.randn(200, 256, device="cuda", generator=gen)
    zs128 = ctx.pack_zs(x[:, :128].contiguous())
    refused(g, x200, zs128, a200, W200, 200, "len_in 200")
    # a graph with a row map
    gm = ctx.graph(rp, ci)
    rmap = torch.arange(n, dtype=torch.int32, device="cuda")
    capi._check(ctx.lib.gaib_graph_set_row_map(ctx.h, gm.h, rmap.data_ptr(), n), "gaib_graph_set_row_map")
    refused(gm, x, zs, agg, W, 256, "row map")
    gm.close()
    # the plain call
    assert ctx.lib.gaib_spmm_gemm_zs_route(ctx.h, g.h, capi.W_GCN, 256, p(x), p(zs), p(agg), None, 256, p(out)) == 0
    assert ctx.lib.gaib_spmm_gemm_zs_route(ctx.h, g.h, capi.W_MEAN_T, 256, p(x), p(zs), p(agg), p(x), 256, p(out)) == 0
    ref_a, ref_o = torch.empty(n, 256, device="cuda"), torch.empty(n, 256, device="cuda")
    ctx.spmm_gemm(g, capi.W_GCN, x, ref_a, W, ref_o)
    assert ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out) is True
    assert torch.equal(bits32(out), bits32(ref_o)) and torch.equal(bits32(agg), bits32(ref_a))
    g.close()


# ---- the layers: agg_zs_wide 1 against 0 --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lctx():
    c = L.init(0)
    yield c
    c.set_option("agg_zs", 1)
    c.set_option("agg_zs_wide", 0)
    c.set_option("agg_bf16", 0)
    c.prof_enable(False)


N_LAYER = 3000


def make_layer(kind, feat_drop=0.0, halo=None, seed=21, width=256):
    rp, ci = random_graph(N_LAYER, 40, seed=seed, power_law=True, hub_deg=1500)
    assert len(ci) >= 12 * N_LAYER  # (rows long enough for the row form: the packed route exists)
    g = L.LGraph.from_host(rp, ci, add_selfloop=(kind == L.GCN))
    if halo is not None:
        g.set_halo(halo, lambda n, p: None, lambda n: 0)
        g.set_partition_mode(L.LGraph.PART_SPLIT)
    layer = L.Layer(kind, 1, N_LAYER, width, width, g, True, feat_drop=feat_drop)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    layer.write(L.FEAT_IN, torch.randn(N_LAYER, width, device="cuda", generator=gen))
    out = torch.empty(N_LAYER, width, device="cuda")
    layer.forward(out)
    L.sync()
    gin = torch.randn(N_LAYER, width, device="cuda", generator=gen)
    return g, layer, out, gin


def backward(lctx, layer, kind, out, gin, width=256):
    """one backward from the same state: (grad_out, weight gradients, the masked grad_in), and the profile's keys"""
    layer.write(L.GRAD_IN, gin)
    grad_out = torch.zeros(N_LAYER, width, device="cuda")
    lctx.prof_reset()
    layer.backward(out, grad_out)
    L.sync()
    res = [grad_out, layer.tensor(L.W_NEIGH_GRAD, (width, width)), layer.tensor(L.GRAD_IN, (N_LAYER, width))]
    if kind == L.SAGE:
        res.append(layer.tensor(L.W_SELF_GRAD, (width, width)))
    return res, set(lctx.prof_table())


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(bits32(x), bits32(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("feat_drop", [0.0, 0.5], ids=["plain", "dropout"])
@pytest.mark.parametrize("kind", [L.GCN, L.SAGE], ids=["gcn", "sage"])
def test_layers_same_bits_with_packed_wide_gradients(lctx, kind, feat_drop):
    g, layer, out, gin = make_layer(kind, feat_drop)
    lctx.prof_enable(True)
    try:
        kept = float((out > 0).float().mean())
        assert 0.3 < kept < 0.7, kept
        lctx.set_option("agg_zs", 1)
        lctx.set_option("agg_zs_wide", 0)
        ref, keys = backward(lctx, layer, kind, out, gin)
        assert "pack_zs_wide" not in keys and "pack_zs" not in keys
        lctx.set_option("agg_zs_wide", 1)
        got, keys = backward(lctx, layer, kind, out, gin)
        assert "pack_zs_wide" in keys and "pack_zs" not in keys, "GCN and SAGE both pack a 256-column gradient"
        assert lctx.get_option("agg_zs_paused") == 0
        assert same_bits(got, ref)
        # the masked gradient is what the dense layer leaves: zeros exactly where the output was cut
        assert bool(((got[2] == 0) | (out > 0)).all())
        lctx.set_option("agg_zs", 0)  # ... overrides the option
        got, keys = backward(lctx, layer, kind, out, gin)
        assert "pack_zs_wide" not in keys and same_bits(got, ref)
    finally:
        lctx.set_option("agg_zs", 1)
        lctx.set_option("agg_zs_wide", 0)
        lctx.prof_enable(False)
        layer.close()
        g.close()


def test_narrow_layer_keeps_its_pack(lctx):
    g, layer, out, gin = make_layer(L.GCN, width=128)
    lctx.prof_enable(True)
    try:
        for wide in (0, 1):
            lctx.set_option("agg_zs_wide", wide)
            _, keys = backward(lctx, layer, L.GCN, out, gin, width=128)
            assert "pack_zs" in keys and "pack_zs_wide" not in keys, wide
    finally:
        lctx.set_option("agg_zs_wide", 0)
        lctx.prof_enable(False)
        layer.close()
        g.close()


def test_not_packed_under_bf16_or_with_a_halo(lctx):
    lctx.prof_enable(True)
    lctx.set_option("agg_zs_wide", 1)
    try:
        g, layer, out, gin = make_layer(L.GCN)
        lctx.set_option("agg_bf16", 1)
        _, keys = backward(lctx, layer, L.GCN, out, gin)
        lctx.set_option("agg_bf16", 0)
        assert "pack_zs_wide" not in keys and "pack_zs" not in keys
        layer.close()
        g.close()
        halo = lctx.graph(np.zeros(N_LAYER + 1, np.int64), np.zeros(0, np.uint32), ncols=1)
        g, layer, out, gin = make_layer(L.SAGE, halo=halo)
        _, keys = backward(lctx, layer, L.SAGE, out, gin)
        assert "pack_zs_wide" not in keys and "pack_zs" not in keys
        layer.close()
        g.close()
    finally:
        lctx.set_option("agg_bf16", 0)
        lctx.set_option("agg_zs_wide", 0)
        lctx.prof_enable(False)


def test_guard_stops_and_resumes(lctx):
    """a gradient that keeps about 90 % of its entries (every half row over capacity: the count is twice the rows): packing stops
    within a few steps, resumes when the density falls, and the outputs are those of the dense layer throughout"""
    g, layer, out50, gin = make_layer(L.GCN, seed=33)
    gen = torch.Generator(device="cuda").manual_seed(34)
    out90 = (torch.rand(N_LAYER, 256, device="cuda", generator=gen) < 0.9).float()
    lctx.prof_enable(True)
    try:
        lctx.set_option("agg_zs_wide", 0)
        ref90, _ = backward(lctx, layer, L.GCN, out90, gin)
        ref50, _ = backward(lctx, layer, L.GCN, out50, gin)
        lctx.set_option("agg_zs_wide", 1)
        got, keys = backward(lctx, layer, L.GCN, out50, gin)
        assert "pack_zs_wide" in keys and same_bits(got, ref50) and lctx.get_option("agg_zs_paused") == 0
        paused_at = None
        packs = 0
        for step in range(12):
            got, keys = backward(lctx, layer, L.GCN, out90, gin)
            assert same_bits(got, ref90), step
            packs += int("pack_zs_wide" in keys)
            if paused_at is None and lctx.get_option("agg_zs_paused") == 1:
                paused_at = step
        assert paused_at is not None and paused_at <= 3, paused_at
        assert packs <= 4, packs  # (the first steps, then one look at the count every eighth call)
        resumed_at = None
        for step in range(24):
            got, keys = backward(lctx, layer, L.GCN, out50, gin)
            assert same_bits(got, ref50), step
            if resumed_at is None and lctx.get_option("agg_zs_paused") == 0:
                resumed_at = step
        assert resumed_at is not None and resumed_at <= 10, resumed_at
        got, keys = backward(lctx, layer, L.GCN, out50, gin)
        assert "pack_zs_wide" in keys and same_bits(got, ref50)
    finally:
        lctx.set_option("agg_zs_wide", 0)
        lctx.prof_enable(False)
        layer.close()
        g.close()


# ---- the trainer --------------------------------------------------------------------------------------------------------
WIDE_LINE = "relu-masked gradients of 256 columns are gathered"


def test_trainer_switch(tmp_path):
    root = make_dataset(tmp_path)
    exe = ROOT / "bin" / "gpu_train_gcn"
    assert exe.exists(), "run graphaibench_amd.build"
    cmd = [str(exe), "cora", "6", "2", "softmax", "256", "0", "0", "0.01", "2", "0", "3", "0"]
    clean = {k: v for k, v in os.environ.items() if k != "GAIB_AGG_ZS_WIDE"}
    runs = {}
    for v in ("1", "0", None):
        env = dict(clean, DATASET_PATH=root, GAIB_EPOCH_GRAPH="0", GAIB_EPOCH_LOSSES="1")
        if v is not None:
            env["GAIB_AGG_ZS_WIDE"] = v
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "relu-masked gradients of 128 columns are gathered zero-suppressed (agg_zs = 1)" in r.stdout
        assert (WIDE_LINE + " zero-suppressed (agg_zs_wide = 1)" in r.stdout) == (v == "1"), r.stdout[-2000:]
        assert (WIDE_LINE in r.stdout) == (v == "1")
        m = re.search(r"epoch_losses ([0-9eE.+\- ]+)", r.stdout + r.stderr)
        assert m, r.stdout[-2000:] + r.stderr[-2000:]
        runs[v] = m.group(1).split()
        assert len(runs[v]) == 6
    assert runs["1"] == runs["0"] == runs[None], runs  # the same bits: the same digits
    env = dict(clean, DATASET_PATH=root, GAIB_AGG_ZS_WIDE="2")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "GAIB_AGG_ZS_WIDE" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
