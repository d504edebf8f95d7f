"""GPU suite, the one-sweep GAT with attention dropout on multi-head rows wider than 128 columns (context options gat_fused_wide
and gat_fused_drop together; gaib_gat_forward_fused_drop_win / gaib_gat_backward_fused_drop_win).  A slab of Hs heads reaches its
masks through a window of the full row's [ne][heads] mask index: element e * mask_heads + mask_head0 + k.  Checked here: the mask
against a numpy port of the library's counter RNG; the full window against the _drop calls and every slab of a wide dropped call
against the _win call on contiguous copies, bit for bit; the results against the staged formulas in fp64 under the library's own
[ne][heads] mask (a wrong head offset or stride gives an unrelated mask and misses by orders of magnitude); an index beyond 2^32;
the refusals; the GAT layer and the trainer with both switches.

The fp64 comparisons use the graphs and the data of tests/test_gpu_gat_drop.py (every pre-activation score stays clear of 0, where
leaky-relu' jumps); the bit identities use the graph of tests/test_gpu_gat_wide.py (333 rows: a hub row of 6 chunks, rows of
exactly 64 and 65 edges, two empty rows)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import test_gpu_bf16 as tb  # helpers (imported as modules: their tests are collected there, not here)
import test_gpu_gat_drop as td
import test_gpu_gat_wide as tw
from graphaibench_amd import capi, layers as L
from oracle import binding as orc
from test_gpu_bf16 import lctx  # noqa: F401  (fixture)
from util import LONG_SUM_FLOOR, assert_close, random_graph

pytestmark = pytest.mark.gpu
ROOT = tb.ROOT
bits32, dev, feat = tb.bits32, tb.dev, tb.feat

RATE, SCALE, SEED = td.RATE, td.SCALE, td.SEED
SENTINEL = tw.SENTINEL
WIDE_SHAPES = [(256, 8), (256, 64), (512, 8), (192, 6), (160, 5), (1024, 16)]  # all three slab widths, Hs = 1, LH = 1, 5 and 6 heads
FWD, BWD = ("out", "row_stats"), ("grad_out", "alpha_lgrad", "alpha_rgrad")
DEFAULTS = dict(gat_fused_wide=0, gat_chunk_xcd=0, gat_fused_unroll=4, gat_fused_fwd=-1, gat_fused_bwd=-1)


# ---- 1. the mask in numpy -------------------------------------------------------------------------------------------------------
def u01_np(seed, index):
    """u01(seed, index) of csrc/common.h over a uint64 index array: splitmix64 of seed + GOLD (index + 1), 24 bits -> [0, 1)"""
    z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (index.astype(np.uint64) + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return ((z ^ (z >> np.uint64(31))) >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def window_mask(ne, heads, seed, mask_heads, mask_head0):
    """[ne][heads]: the masks of elements e * mask_heads + mask_head0 + k of a virtual [ne][mask_heads] array"""
    index = np.arange(ne, dtype=np.uint64)[:, None] * np.uint64(mask_heads) + np.uint64(mask_head0) + np.arange(heads, dtype=np.uint64)[None, :]
    return (u01_np(seed, index) > np.float32(RATE)).astype(np.uint8)


@pytest.mark.parametrize("heads", [5, 8])
def test_the_mask_in_numpy(ctx, heads):
    ne = 20_011
    lib = td.library_mask(ctx, ne, heads, SEED)
    assert np.array_equal(window_mask(ne, heads, SEED, heads, 0), lib)
    # a window of the same array: heads [2, 5) of the row
    assert np.array_equal(window_mask(ne, 3, SEED, heads, 2), lib[:, 2:5])


# ---- helpers: the calls on sentinel-filled outputs ----------------------------------------------------------------------------------
@pytest.fixture
def graph(ctx):
    rp, ci = tw.host_graph()
    g = ctx.graph(rp, ci.view(np.int32))
    yield g
    g.close()


@pytest.fixture
def wide(ctx):
    """gat_fused_wide on; every knob a test may turn goes back to its default afterwards"""
    assert ctx.get_option("gat_fused_wide") == 0  # ships off
    ctx.set_option("gat_fused_wide", 1)
    yield ctx
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)


def filled(*shape):
    return torch.full(shape, SENTINEL, device="cuda")


def forward(ctx, g, h, al, ar, heads, rate=RATE, scale=None, seed=SEED, relu=False, win=None):
    """win = (mask_heads, mask_head0): the _win call; rate None: the undropped call"""
    n, d = h.shape
    out, stats = filled(n, d), filled(n, heads, 2)
    if rate is None:
        ok = ctx.gat_forward_fused(g, h, al, ar, out, stats, heads=heads, relu=relu)
    elif win is None:
        ok = ctx.gat_forward_fused_drop(g, h, al, ar, out, stats, rate, seed, scale=scale, heads=heads, relu=relu)
    else:
        ok = ctx.gat_forward_fused_drop_win(g, h, al, ar, out, stats, rate, seed, win[0], win[1], scale=scale, heads=heads, relu=relu)
    ctx.sync()
    assert ok, "refused"
    return dict(out=out, row_stats=stats)


def backward(ctx, g, h, gin, fwd_out, al, ar, stats, heads, rate=RATE, scale=None, seed=SEED, win=None):
    n, d = h.shape
    go, lg, rg = filled(n, d), filled(d), filled(d)
    if rate is None:
        ok = ctx.gat_backward_fused(g, h, gin, fwd_out, al, ar, None, go, lg, rg, heads=heads, row_stats=stats)
    elif win is None:
        ok = ctx.gat_backward_fused_drop(g, h, gin, fwd_out, al, ar, go, lg, rg, stats, rate, seed, scale=scale, heads=heads)
    else:
        ok = ctx.gat_backward_fused_drop_win(g, h, gin, fwd_out, al, ar, go, lg, rg, stats, rate, seed, win[0], win[1], scale=scale,
                                             heads=heads)
    ctx.sync()
    assert ok, "refused"
    return dict(grad_out=go, alpha_lgrad=lg, alpha_rgrad=rg)


def both(ctx, g, ins, heads, **kw):
    h, gin, al, ar = ins
    f = forward(ctx, g, h, al, ar, heads, **kw)
    kw.pop("relu", None)
    res = {**f, **backward(ctx, g, h, gin, f["out"], al, ar, f["row_stats"], heads, **kw)}
    for name, t in res.items():
        assert torch.isfinite(t).all() and not bool((t == SENTINEL).any()), name
    return res


def same(a, b, what, names=FWD + BWD):
    for name in names:
        tw.same(a[name], b[name], f"{what}: {name}")


# ---- 2. the full window is the _drop call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,heads", [(32, 1), (32, 8), (64, 2), (64, 16), (128, 4), (128, 16)])  # every G, LH = 1 and LH > 1
def test_full_window_has_the_bits_of_the_drop_call(ctx, graph, d, heads):
    ins = tuple(dev(a) for a in tw.host_case(d))
    drop = both(ctx, graph, ins, heads, relu=True)
    win = both(ctx, graph, ins, heads, relu=True, win=(heads, 0))
    same(win, drop, f"({d}, {heads}) window (heads, 0)")
    assert not torch.equal(drop["out"], both(ctx, graph, ins, heads, relu=True, win=(heads + 3, 1))["out"])  # (another window: other masks)


# ---- 3. every slab of a wide dropped call is the _win call on contiguous copies -----------------------------------------------------
def slab_calls(ctx, g, ins, wide_res, d, heads, what, fwd_only=False, **kw):
    """the _win calls at (w, Hs, heads, s Hs) on contiguous copies of slab s, held against the wide call's columns and heads"""
    w, S, Hs = tw.slabs(d, heads)
    h, gin, al, ar = ins
    for s in range(S):
        c, hd = slice(s * w, (s + 1) * w), slice(s * Hs, (s + 1) * Hs)
        cut = lambda t: t[:, c].contiguous()  # noqa: E731
        f = forward(ctx, g, cut(h), al[c].contiguous(), ar[c].contiguous(), Hs, win=(heads, s * Hs), **kw)
        tw.same(wide_res["out"][:, c], f["out"], f"{what}: out, slab {s}")
        tw.same(wide_res["row_stats"][:, hd], f["row_stats"], f"{what}: row_stats, slab {s}")
        if fwd_only:
            continue
        kb = {k: v for k, v in kw.items() if k != "relu"}
        # (backward on the wide call's forward output and statistics: the slab's inputs are then the wide call's bits)
        b = backward(ctx, g, cut(h), cut(gin), cut(wide_res["out"]), al[c].contiguous(), ar[c].contiguous(),
                     wide_res["row_stats"][:, hd].contiguous(), Hs, win=(heads, s * Hs), **kb)
        tw.same(wide_res["grad_out"][:, c], b["grad_out"], f"{what}: grad_out, slab {s}")
        tw.same(wide_res["alpha_lgrad"][c], b["alpha_lgrad"], f"{what}: alpha_l gradient, slab {s}")
        tw.same(wide_res["alpha_rgrad"][c], b["alpha_rgrad"], f"{what}: alpha_r gradient, slab {s}")


@pytest.mark.parametrize("d,heads", WIDE_SHAPES)
def test_slab_identity(wide, graph, d, heads):
    ctx = wide
    ins = tuple(dev(a) for a in tw.host_case(d))
    h, gin, al, ar = ins
    what = f"({d}, {heads})"
    plain = both(ctx, graph, ins, heads, rate=None)
    dropped = both(ctx, graph, ins, heads)
    slab_calls(ctx, graph, ins, dropped, d, heads, what)
    slab_calls(ctx, graph, ins, forward(ctx, graph, h, al, ar, heads, relu=True), d, heads, what + " relu", fwd_only=True, relu=True)
    same(dropped, plain, what + ": the softmax statistics do not see the mask", names=("row_stats",))
    for name in ("out", "grad_out", "alpha_lgrad", "alpha_rgrad"):
        assert not torch.equal(dropped[name], plain[name]), name
    same(both(ctx, graph, ins, heads, rate=0.0, scale=1.0), plain, what + ": rate 0, scale 1 against the undropped wide call")
    same(both(ctx, graph, ins, heads), dropped, what + ": the same seed again")
    other = both(ctx, graph, ins, heads, seed=SEED + 1)
    assert not torch.equal(other["out"], dropped["out"]) and not torch.equal(other["grad_out"], dropped["grad_out"])
    for v in tw.ISOLATED:  # an empty row: zeros
        assert bool((dropped["out"][v] == 0).all()) and bool((dropped["row_stats"][v, :, 1] == 0).all())
        assert bool((dropped["grad_out"][v] == 0).all())
    # backward under the launch options the wide path honours (333 rows: 85 workgroups, the XCD walk engages)
    cases = [dict(gat_chunk_xcd=1)] + ([dict(gat_fused_unroll=8)] if (d, heads) == (192, 6) else [])
    for opts in cases:
        for k, v in opts.items():
            ctx.set_option(k, v)
        under = {**dropped, **backward(ctx, graph, h, gin, dropped["out"], al, ar, dropped["row_stats"], heads)}
        slab_calls(ctx, graph, ins, under, d, heads, f"{what} {opts}")
        for k in opts:
            ctx.set_option(k, DEFAULTS[k])


# ---- 4. against the staged formulas in fp64, under the library's [ne][heads] mask -------------------------------------------------
def check_fp64(res, g_o, rows, col, ins_host, heads, mask, what):
    h, gin, al, ar = ins_host
    want, T, wlg, wrg = td.expectation(g_o, rows, col, h, al, ar, heads, mask, lambda _w: gin, relu=False)
    assert_close(res["out"].cpu().numpy(), want, what + " forward", floor=LONG_SUM_FLOOR)
    assert_close(res["grad_out"].cpu().numpy(), T, what + " grad_out", floor=LONG_SUM_FLOOR)
    assert_close(res["alpha_lgrad"].cpu().numpy(), wlg, what + " alpha_l grad", floor=LONG_SUM_FLOOR)
    assert_close(res["alpha_rgrad"].cpu().numpy(), wrg, what + " alpha_r grad", floor=LONG_SUM_FLOOR)


@pytest.mark.parametrize("gname", list(td.GRAPHS))
@pytest.mark.parametrize("d,heads", [(256, 8), (160, 5)])
def test_against_the_staged_formulas_in_fp64(wide, gname, d, heads):
    ctx = wide
    _, _, g_o, rows, col = td.host_graph(gname)
    g, ins = td.device_case(ctx, gname, d, heads)
    try:
        res = both(ctx, g, ins, heads)
        mask = td.library_mask(ctx, g_o.ne, heads, SEED)
        check_fp64(res, g_o, rows, col, td.case(gname, d, heads), heads, mask, f"{gname} {d} x {heads}")
    finally:
        g.close()


# ---- 5. the index in 64 bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,heads", [(32, 8), (128, 4)])
def test_the_index_is_formed_in_64_bits(ctx, d, heads):
    _, _, g_o, rows, col = td.host_graph("hub")
    mask_heads = 1 << 22
    mask_head0 = mask_heads - heads  # e * 2^22 + 2^22 - heads + k: beyond 2^32 from edge 1 024 on
    assert g_o.ne > 4096 and 1024 * mask_heads + mask_head0 >= 1 << 32
    mask = window_mask(g_o.ne, heads, SEED, mask_heads, mask_head0)
    assert abs(1.0 - mask.mean() - RATE) < 5 * np.sqrt(RATE * (1 - RATE) / mask.size)
    # (the index taken mod 2^32 gives another mask: the comparison below would not pass with it)
    index = np.arange(g_o.ne, dtype=np.uint64)[:, None] * np.uint64(mask_heads) + np.uint64(mask_head0) + np.arange(heads, dtype=np.uint64)[None, :]
    assert (mask != (u01_np(SEED, index & np.uint64(0xFFFFFFFF)) > np.float32(RATE))).mean() > 0.3
    g, ins = td.device_case(ctx, "hub", d, heads)
    try:
        res = both(ctx, g, ins, heads, win=(mask_heads, mask_head0))
        check_fp64(res, g_o, rows, col, td.case("hub", d, heads), heads, mask, f"hub {d} x {heads}, window at 2^22 - {heads}")
    finally:
        g.close()


# ---- 6. refusals leave the outputs untouched ----------------------------------------------------------------------------------------
def attempt(ctx, g, d, heads, offset=0, rate=RATE, stats_none=False, rows=tw.NV, win=None):
    """(forward accepted, backward accepted, forward's outputs untouched, backward's outputs untouched); a call that must raise
    GaibError counts as not accepted"""
    NV = tw.NV
    gen = torch.Generator(device="cuda").manual_seed(d + heads)
    flat = torch.randn(rows * d + 8, device="cuda", generator=gen)
    h = flat[offset:offset + rows * d].view(rows, d)
    gin, fwd_out = torch.randn(rows, d, device="cuda", generator=gen), torch.randn(NV, d, device="cuda", generator=gen)
    al, ar = torch.randn(d, device="cuda", generator=gen), torch.randn(d, device="cuda", generator=gen)
    st = torch.rand(NV, heads, 2, device="cuda", generator=gen) + 0.5
    out, stats = filled(NV, d), filled(NV, heads, 2)
    go, lg, rg = filled(NV, d), filled(d), filled(d)
    if win is None:
        fcall = lambda: ctx.gat_forward_fused_drop(g, h, al, ar, out, stats, rate, SEED, scale=1.0, heads=heads)  # noqa: E731
        bcall = lambda: ctx.gat_backward_fused_drop(g, h, gin, fwd_out, al, ar, go, lg, rg, None if stats_none else st, rate, SEED,  # noqa: E731
                                                    scale=1.0, heads=heads)
    else:
        fcall = lambda: ctx.gat_forward_fused_drop_win(g, h, al, ar, out, stats, rate, SEED, win[0], win[1], scale=1.0, heads=heads)  # noqa: E731
        bcall = lambda: ctx.gat_backward_fused_drop_win(g, h, gin, fwd_out, al, ar, go, lg, rg, st, rate, SEED, win[0], win[1],  # noqa: E731
                                                        scale=1.0, heads=heads)
    raises = rate >= 1.0 or stats_none or (win is not None and (win[1] < 0 or win[1] + heads > win[0]))
    if raises:
        f = b = False
        if not stats_none:  # (forward has no business with the statistics argument of backward)
            with pytest.raises(capi.GaibError):
                fcall()
        with pytest.raises(capi.GaibError):
            bcall()
    else:
        f, b = fcall(), bcall()
    ctx.sync()
    untouched = lambda ts: all(bool((t == SENTINEL).all()) for t in ts)  # noqa: E731
    return f, b, untouched((out, stats)), untouched((go, lg, rg))


def test_refusals_leave_the_outputs_untouched(ctx, graph):
    rp, ci = tw.host_graph()
    refused = (False, False, True, True)
    assert ctx.get_option("gat_fused_wide") == 0
    for d, heads in WIDE_SHAPES:  # option 0: what these shapes always returned
        assert attempt(ctx, graph, d, heads) == refused, (d, heads)
    rect = ctx.graph(rp, ci.view(np.int32), ncols=tw.NV + 40)
    try:
        ctx.set_option("gat_fused_wide", 1)
        assert attempt(ctx, graph, 256, 8) == (True, True, False, False)  # (the accepted call, for contrast)
        assert attempt(ctx, graph, 256, 1) == refused  # a single head wider than 128 columns
        assert attempt(ctx, graph, 200, 8) == refused  # no slab width divides it
        assert attempt(ctx, graph, 256, 8, offset=1) == refused  # the table 4 bytes off its alignment
        assert attempt(ctx, rect, 256, 8, rows=tw.NV + 40) == refused  # a rectangular graph
        assert attempt(ctx, graph, 256, 8, rate=1.0) == refused  # GaibError
        assert attempt(ctx, graph, 256, 8, stats_none=True) == refused  # GaibError from backward; forward is not called
        ctx.set_option("gat_fused_fwd", 0)
        assert attempt(ctx, graph, 256, 8) == (False, True, True, False)
        ctx.set_option("gat_fused_fwd", -1)
        ctx.set_option("gat_fused_bwd", 0)
        assert attempt(ctx, graph, 256, 8) == (True, False, False, True)
        ctx.set_option("gat_fused_bwd", -1)
        # the window calls: a window that is none -> GaibError; else the _drop calls' answers
        assert attempt(ctx, graph, 64, 4, win=(8, 4)) == (True, True, False, False)  # heads [4, 8) of 8
        assert attempt(ctx, graph, 64, 4, win=(8, 5)) == refused
        assert attempt(ctx, graph, 64, 4, win=(3, 0)) == refused
        assert attempt(ctx, graph, 64, 4, win=(8, -1)) == refused
        assert attempt(ctx, graph, 256, 8, win=(8, 0)) == refused  # (not a narrow shape: the wide form is the _drop call's)
        assert attempt(ctx, graph, 64, 4, win=(8, 4), offset=1) == refused
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)
        rect.close()


# ---- 7. the layer -------------------------------------------------------------------------------------------------------------------
DIN, DOUT, HEADS = 48, 256, 8
FIRST_SEED = td.FIRST_SEED


def holds_arrays(ly):
    return [k for k in (L.NORM_SCORES_GRAD, L.ATTN_MASKS, L.NORM_SCORES_DROPPED) if ly.ld.ptr(k) not in (0, None)]


def test_layer_with_both_options(lctx):
    rp, ci, g_o, rows, col = td.host_graph("hub")
    n, ne = g_o.nv, g_o.ne
    W = orc.init_glorot(DIN, DOUT, 1)
    al, ar = orc.init_glorot(DOUT, 1, 2).ravel(), orc.init_glorot(DOUT, 1, 3).ravel()
    x = td.off_zero(feat(n, DIN, 3), W.astype(np.float64), al, ar, HEADS)
    gin = feat(n, DOUT, 4)
    hfeat = orc.matmul(x, W)
    mask = td.library_mask(lctx, ne, HEADS, FIRST_SEED)
    want, T, lg, rg = td.expectation(g_o, rows, col, hfeat, al, ar, HEADS, mask, lambda w: np.where(w > 0, gin, 0), relu=True)
    g_d = L.LGraph.from_host(rp, ci, add_selfloop=True)
    assert lctx.get_option("gat_fused_drop") == 0 and lctx.get_option("gat_fused_wide") == 0  # the defaults
    layers = []

    def layer(score_drop=RATE):
        if score_drop:
            layers.append(td.DropLayer(g_d, n, DIN, DOUT, HEADS, x))
        else:
            ly = tw.WideLayer(g_d, n, dev(x))
            ly.forward_phase = lambda phase: (ly.ld.set_phase(phase), ly.forward())[1]
            layers.append(ly)
        return layers[-1]

    def grads(ly):
        return (ly.grad_out.clone(), ly.ld.tensor(L.W_NEIGH_GRAD, (DIN, DOUT)).clone(), ly.ld.tensor(L.ALPHA_LGRAD, (DOUT,)).clone(),
                ly.ld.tensor(L.ALPHA_RGRAD, (DOUT,)).clone())

    try:
        # both options 0: the staged path
        staged = layer()
        out0 = staged.forward(0)
        staged.backward(want, gin)
        g0 = grads(staged)
        assert_close(out0.cpu().numpy(), want, "staged training forward", floor=LONG_SUM_FLOOR)
        assert len(holds_arrays(staged)) == 3
        # gat_fused_drop alone: nothing changes at this width
        lctx.set_option("gat_fused_drop", 1)
        drop_only = layer()
        tw.same(drop_only.forward(0), out0, "gat_fused_drop alone: feat_out")
        drop_only.backward(want, gin)
        for a, b, name in zip(grads(drop_only), g0, ("grad_out", "W_neigh_grad", "alpha_l grad", "alpha_r grad")):
            tw.same(a, b, "gat_fused_drop alone: " + name)
        # both options 1: the one sweep per slab
        lctx.set_option("gat_fused_wide", 1)
        sweep, fallback, undropped = layer(), layer(), layer(score_drop=0.0)
        assert holds_arrays(sweep) == []
        tw.same(sweep.forward(1), undropped.forward_phase(1), "a test-phase forward drops nothing")
        out1 = sweep.forward(0)
        assert_close(out1.cpu().numpy(), want, "one-sweep training forward", floor=LONG_SUM_FLOOR)
        assert_close(out1.cpu().numpy(), out0.cpu().numpy(), "one-sweep training forward against the staged layer")
        sweep.backward(want, gin)
        sweep.check(x, W, T, lg, rg, "one sweep")
        for a, b, name in zip(grads(sweep), g0, ("grad_out", "W_neigh_grad", "alpha_l grad", "alpha_r grad")):
            assert_close(a.cpu().numpy(), b.cpu().numpy(), "against the staged layer: " + name, floor=LONG_SUM_FLOOR)
        assert holds_arrays(sweep) == []  # no [ne][heads] array, mask or dropped attention was allocated on the way
        assert not torch.equal(sweep.forward(0), out1)  # the next seed
        # forward in the sweep, backward not allowed to: the staged pieces on the remembered seed, allocated on demand
        tw.same(fallback.forward(0), out1, "the same forward")
        lctx.set_option("gat_fused_bwd", 0)
        fallback.backward(want, gin)
        lctx.set_option("gat_fused_bwd", -1)
        fallback.check(x, W, T, lg, rg, "staged fallback")
        assert len(holds_arrays(fallback)) == 3
    finally:
        for k, v in dict(gat_fused_bwd=-1, gat_fused_drop=0, gat_fused_wide=0).items():
            lctx.set_option(k, v)
        for ly in layers:
            ly.ld.close()
        g_d.close()


def test_layer_holds_less_device_memory_with_both_options(lctx):
    """as tests/test_gpu_gat_wide.py::test_layer_holds_less_device_memory_with_the_option, under dropout: held after construction
    and one training step -- lower with both options by at least one [ne][heads] fp32 array (staged: three of them, the mask, the
    dropped attention and a workspace)"""
    n = 40_000
    rp, ci = random_graph(n, 24, seed=5, power_law=True, hub_deg=2000)
    x, gin = torch.randn(n, DIN, device="cuda"), torch.randn(n, DOUT, device="cuda")

    def free_bytes():
        L.sync()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def held(option):
        lctx.set_option("gat_fused_wide", option)
        lctx.set_option("gat_fused_drop", option)
        before = free_bytes()
        g_d = L.LGraph.from_host(rp, ci, add_selfloop=True)
        ly = tw.WideLayer(g_d, n, x, score_drop=RATE)
        ly.backward(ly.forward(), gin)
        ne = g_d.ne
        h = before - free_bytes()
        ly.ld.close()
        g_d.close()
        return h, ne

    try:
        held(1)  # the context's workspace and torch's allocator reach their size for the option-1 step
        h1, ne = held(1)
        h0, _ = held(0)
    finally:
        lctx.set_option("gat_fused_wide", 0)
        lctx.set_option("gat_fused_drop", 0)
    array = ne * HEADS * 4
    print(f"held with both options {h1 / 2**20:.1f} MiB, without {h0 / 2**20:.1f} MiB, one [ne][heads] array {array / 2**20:.1f} MiB")
    assert array > 16 << 20  # (far above the allocator's granularity)
    assert h0 - h1 >= array, (h0, h1, array)


# ---- 8. the trainer -----------------------------------------------------------------------------------------------------------------
PARITY_BAR, TRAINER_BAR = td.PARITY_BAR, td.TRAINER_BAR  # first epoch: same weights and masks; final loss: the project's bars


def train(root, wide_switch, drop_switch):
    exe = ROOT / "bin" / "gpu_train_gat"
    assert exe.exists(), "run graphaibench_amd.build"
    cmd = [str(exe), "cora", "20", "2", "softmax", "256", "0.3", "0", "0.01", "2", "0", "4", "0"]
    env = dict(os.environ, DATASET_PATH=root, GAIB_GAT_HEADS="8", GAIB_EPOCH_LOSSES="1", GAIB_GAT_WIDE=wide_switch,
               GAIB_GAT_FUSED_DROP=drop_switch)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"epoch_losses ([0-9eE.+\- ]+)", r.stdout + r.stderr)
    assert m, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(v) for v in m.group(1).split()]
    assert len(losses) == 20 and np.isfinite(losses).all(), losses
    return r.stdout, losses


def test_trainer_with_both_switches(tmp_path):
    root = tb.make_dataset(tmp_path)
    out0, s = train(root, "0", "0")
    assert out0.count("GAT wide rows:") == 0 and out0.count("GAT attention dropout: staged") == 1, out0[-2000:]
    out1, o = train(root, "1", "1")
    for line in ("GAT wide rows: one sweep, 2 slabs of 128", "GAT attention dropout: one sweep"):
        assert out1.count(line) == 1, out1[-2000:]
    assert out1.count("GAT wide rows:") == 1 and out1.count("GAT attention dropout:") == 1, out1[-2000:]
    outw, _ = train(root, "1", "0")
    for line in ("GAT wide rows: staged", "GAT attention dropout: staged"):
        assert outw.count(line) == 1, outw[-2000:]
    assert outw.count("GAT wide rows:") == 1 and outw.count("GAT attention dropout:") == 1, outw[-2000:]
    print(f"first loss staged {s[0]:.7f} one sweep {o[0]:.7f} rel {abs(o[0] - s[0]) / s[0]:.3e}; "
          f"final {s[-1]:.6f} {o[-1]:.6f} rel {abs(o[-1] - s[-1]) / s[-1]:.3e}")
    assert abs(o[0] - s[0]) <= PARITY_BAR * s[0], (o[0], s[0])
    assert abs(o[-1] - s[-1]) <= TRAINER_BAR * s[-1], (o[-1], s[-1])
