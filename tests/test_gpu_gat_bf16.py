"""GPU suite, the one-sweep GAT forward and backward over bf16 tables (gaib_gat_forward_fused_bf16 /
gaib_gat_backward_fused_bf16): bit for bit against the fp32 calls on the widened tables at every row width and under every
option the fp32 calls honour, the refusals, the profile rows, the GAT layer with the context option gat_bf16 against the fp32
layer on representable data, the refusal on a partition, and the trainer with GAIB_GAT_DTYPE=bf16."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_bf16 as tb  # helpers of the plain bf16 suite (imported as a module: its tests are collected there, not here)
from graphaibench_amd import capi, layers as L
from test_gpu_bf16 import lctx  # noqa: F401  (fixture)
from util import random_graph

pytestmark = pytest.mark.gpu
ROOT = tb.ROOT
bits32 = tb.bits32

SHAPES = [(32, 1, 0), (32, 8, 900), (32, 4, 0), (64, 1, 900), (64, 8, 0), (64, 16, 0), (128, 1, 0), (128, 8, 1400), (128, 16, 0),
          (128, 2, 700)]


def hub_graph(ctx, d, heads, hub):
    rp, ci = random_graph(1300, 7, seed=3 * d + heads, power_law=True, hub_deg=hub)
    return ctx.graph(rp, ci.view(np.int32)).add_selfloop(), len(rp) - 1


def table(n, d, gen):
    """a random bf16 table with a row of +0.0, one of -0.0 and one of bf16 subnormals"""
    t = torch.randn(n, d, device="cuda", generator=gen).to(torch.bfloat16)
    w = t.view(torch.int16)
    w[3] = 0
    w[5] = -32768  # 0x8000: -0.0
    w[7] = (torch.arange(d, device="cuda") % 127 + 1).to(torch.int16)  # 0x0001 .. 0x007f: subnormals
    w[8] = w[7] | -32768
    return t


def inputs(ctx, n, d, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    hb, gb = table(n, d, gen), table(n, d, gen)
    al = torch.randn(d, device="cuda", generator=gen) * 0.2
    ar = torch.randn(d, device="cuda", generator=gen) * 0.2
    return hb, gb, ctx.cast_bf16_f32(hb), ctx.cast_bf16_f32(gb), al, ar


def run_pair(ctx, g, n, d, heads, ins, relu):
    """(fp32 on the widened tables, bf16): out, row_stats, grad_out, alpha_l grad, alpha_r grad -- filled with 7.0 beforehand"""
    hb, gb, hw, gw, al, ar = ins
    res = []
    for bf in (False, True):
        out = torch.full((n, d), 7.0, device="cuda")
        stats = torch.full((n, heads, 2), 7.0, device="cuda")
        go = torch.full((n, d), 7.0, device="cuda")
        lg, rg = torch.full((d,), 7.0, device="cuda"), torch.full((d,), 7.0, device="cuda")
        if bf:
            assert ctx.gat_forward_fused_bf16(g, hb, al, ar, out, stats, heads=heads, relu=relu)
            assert ctx.gat_backward_fused_bf16(g, hb, gb, out, al, ar, go, lg, rg, stats, heads=heads)
        else:
            assert ctx.gat_forward_fused(g, hw, al, ar, out, stats, heads=heads, relu=relu)
            assert ctx.gat_backward_fused(g, hw, gw, out, al, ar, None, go, lg, rg, heads=heads, row_stats=stats)
        res.append((out, stats, go, lg, rg))
    return res


def assert_same(ref, got, what):
    for name, a, b in zip(("out", "row_stats", "grad_out", "alpha_lgrad", "alpha_rgrad"), ref, got):
        assert torch.equal(bits32(a), bits32(b)), (name, what, int((bits32(a) != bits32(b)).sum()))
        assert torch.isfinite(b).all(), (name, what)


# ---- 1. bit identity at every row width -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,heads,hub", SHAPES)
@pytest.mark.parametrize("pk", [0, 1])
def test_bits_of_the_fp32_calls_on_the_widened_tables(ctx, d, heads, hub, pk):
    g, n = hub_graph(ctx, d, heads, hub)
    ins = inputs(ctx, n, d, 100 * d + heads)
    ctx.set_option("gat_bwd_pk", pk)
    try:
        for relu in (False, True):
            ref, got = run_pair(ctx, g, n, d, heads, ins, relu)
            assert_same(ref, got, (d, heads, hub, pk, relu))
            assert not torch.equal(got[2], torch.full_like(got[2], 7.0))
            _, again = run_pair(ctx, g, n, d, heads, ins, relu)
            assert_same(got, again, "second run")
    finally:
        ctx.set_option("gat_bwd_pk", 0)
        g.close()


# ---- 2. the options the fp32 calls honour -----------------------------------------------------------------------------------
VARIANTS = [dict(gat_fused_unroll=4), dict(gat_fused_unroll=8), dict(gat_chunk_xcd=1), dict(gat_interleave=1),
            dict(gat_fused_unroll=8, gat_chunk_xcd=1, gat_interleave=1)]


@pytest.mark.parametrize("d,heads,hub", [(64, 8, 1400), (128, 8, 0)])
def test_variants_keep_the_identity(ctx, d, heads, hub):
    g, n = hub_graph(ctx, d, heads, hub)  # (1 300 rows: at least 325 chunks, grid >= 64 for gat_chunk_xcd)
    ins = inputs(ctx, n, d, 7 * d + heads)
    defaults = dict(gat_fused_unroll=4, gat_chunk_xcd=0, gat_interleave=0)
    try:
        base = None
        for opts in VARIANTS:
            for pk in (0, 1):
                for k, v in {**defaults, **opts, "gat_bwd_pk": pk}.items():
                    ctx.set_option(k, v)
                ref, got = run_pair(ctx, g, n, d, heads, ins, False)
                assert_same(ref, got, (d, heads, opts, pk))
                if pk == 0:  # (the chunk kernel's options change no bits: fixed order of additions)
                    base = base or got
                    assert_same(base, got, ("against the first variant", opts))
    finally:
        for k, v in {**defaults, "gat_bwd_pk": 0}.items():
            ctx.set_option(k, v)
        g.close()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ctx):
    rp, ci = random_graph(300, 6, seed=2)
    n = 300
    g = ctx.graph(rp, ci.view(np.int32)).add_selfloop()
    rect = ctx.graph(rp, ci.view(np.int32), ncols=n + 40)

    def attempt(graph, d, heads=4, offset=0, stats_none=False, rows=n):
        gen = torch.Generator(device="cuda").manual_seed(d)
        flat = torch.randn(rows * d + 8, device="cuda", generator=gen).to(torch.bfloat16)
        hb = flat[offset:offset + rows * d].view(rows, d)
        gb = torch.randn(n, d, device="cuda", generator=gen).to(torch.bfloat16)
        al, ar = torch.randn(d, device="cuda", generator=gen), torch.randn(d, device="cuda", generator=gen)
        out, stats = torch.full((n, d), 7.0, device="cuda"), torch.full((n, heads, 2), 7.0, device="cuda")
        go, lg, rg = torch.full((n, d), 7.0, device="cuda"), torch.full((d,), 7.0, device="cuda"), torch.full((d,), 7.0, device="cuda")
        fwd_out = torch.randn(n, d, device="cuda", generator=gen)
        outs = (out, stats, go, lg, rg)
        if stats_none:
            with pytest.raises(capi.GaibError):
                ctx.gat_backward_fused_bf16(graph, hb, gb, fwd_out, al, ar, go, lg, rg, None, heads=heads)
            f = b = False
        else:
            f = ctx.gat_forward_fused_bf16(graph, hb, al, ar, out, stats, heads=heads)
            st = torch.rand(n, heads, 2, device="cuda", generator=gen) + 0.5
            b = ctx.gat_backward_fused_bf16(graph, hb, gb, fwd_out, al, ar, go, lg, rg, st, heads=heads)
        return f, b, all(bool((t == 7.0).all()) for t in ((go, lg, rg) if f else outs))

    try:
        assert attempt(g, 64) == (True, True, False)  # (the accepted call, for contrast)
        assert attempt(g, 48) == (False, False, True)
        assert attempt(rect, 64, rows=n + 40) == (False, False, True)
        assert attempt(g, 64, offset=1) == (False, False, True)  # the table 2 bytes off its alignment
        assert attempt(g, 64, stats_none=True) == (False, False, True)
        ctx.set_option("gat_fused_fwd", 0)
        f, b, _ = attempt(g, 64)
        assert (f, b) == (False, True)
        ctx.set_option("gat_fused_fwd", -1)
        ctx.set_option("gat_fused_bwd", 0)
        f, b, untouched = attempt(g, 64)
        assert (f, b, untouched) == (True, False, True)
    finally:
        ctx.set_option("gat_fused_fwd", -1)
        ctx.set_option("gat_fused_bwd", -1)
        g.close()
        rect.close()


# ---- 4. the rounding is real; the profile rows --------------------------------------------------------------------------------
def test_rounding_shows_and_profile_rows(ctx):
    d, heads = 64, 8
    g, n = hub_graph(ctx, d, heads, 0)
    gen = torch.Generator(device="cuda").manual_seed(11)
    h = torch.randn(n, d, device="cuda", generator=gen)
    gin = torch.randn(n, d, device="cuda", generator=gen)
    al, ar = torch.randn(d, device="cuda", generator=gen) * 0.2, torch.randn(d, device="cuda", generator=gen) * 0.2
    hb, gb = ctx.cast_f32_bf16(h), ctx.cast_f32_bf16(gin)
    out32, st32 = torch.empty(n, d, device="cuda"), torch.empty(n, heads, 2, device="cuda")
    out16, st16 = torch.empty(n, d, device="cuda"), torch.empty(n, heads, 2, device="cuda")
    assert ctx.gat_forward_fused(g, h, al, ar, out32, st32, heads=heads)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        assert ctx.gat_forward_fused_bf16(g, hb, al, ar, out16, st16, heads=heads)
        go, lg, rg = torch.empty(n, d, device="cuda"), torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
        assert ctx.gat_backward_fused_bf16(g, hb, gb, out16, al, ar, go, lg, rg, st16, heads=heads)
        ctx.sync()
        tab = ctx.prof_table()
    finally:
        ctx.prof_enable(False)
    assert not torch.equal(out16, out32)  # an unrounded h: the bf16 call reads the rounded table, not a widened copy of h
    err = (out16 - out32).abs().max().item()
    assert 0 < err < 2.0 ** -6 * h.abs().max().item(), err  # (a convex combination of rows rounded to 8 bits)
    assert tab["gat_fwd_fused"]["count"] == 1 and tab["gat_bwd_fused"]["count"] == 1, tab
    assert "cast_bf16_f32" not in tab, tab
    g.close()


# ---- 5 / 6. the layer on representable data -----------------------------------------------------------------------------------
def rounded(t):
    return t.to(torch.bfloat16).to(torch.float32)


class GatLayer:
    """a GAT layer 64 -> 64 over cora whose h rows are rows of a bf16-representable W (FEAT_IN: one 1.0 per row, in column
    (v + shift) % d; every layer is created with the same W, so the shift is what makes two layers' h tables differ)"""

    def __init__(self, g_d, seed, shift=0, n=2708, d=64, heads=8):
        self.n, self.d = n, d
        self.ld = L.Layer(L.GAT, 1, n, d, d, g_d, True)
        self.ld.set_heads(heads)
        self.ld.write(L.W_NEIGH, rounded(self.ld.tensor(L.W_NEIGH, (d, d))))
        x = torch.zeros(n, d, device="cuda")
        x[torch.arange(n), (torch.arange(n) + shift) % d] = 1.0
        self.ld.write(L.FEAT_IN, x)
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.gin = rounded(torch.randn(n, d, device="cuda", generator=gen))
        self.out = torch.empty(n, d, device="cuda")
        self.go = torch.zeros(n, d, device="cuda")

    def forward(self):
        self.ld.forward(self.out)

    def backward(self):
        # (the layer's d_relu masks GRAD_IN in place by the forward output: a masked representable value stays representable)
        self.ld.write(L.GRAD_IN, self.gin)
        self.ld.backward(self.out, self.go)

    def result(self):
        L.sync()
        d = self.d
        return dict(out=self.out.clone(), go=self.go.clone(), Wg=self.ld.tensor(L.W_NEIGH_GRAD, (d, d)),
                    lg=self.ld.tensor(L.ALPHA_LGRAD, (d,)), rg=self.ld.tensor(L.ALPHA_RGRAD, (d,)))

    def close(self):
        self.ld.close()


def layer_run(lctx, on, n_layers, profile=False):
    rp, ci = tb.cora()
    g_d = L.LGraph.from_host(rp, ci, add_selfloop=True)
    lctx.set_option("gat_bf16", on)
    tab = None
    try:
        layers = [GatLayer(g_d, 20 + k, shift=5 * k) for k in range(n_layers)]
        if profile:
            lctx.prof_enable(True)
            lctx.prof_reset()
        for ly in layers:
            ly.forward()
        for ly in reversed(layers):
            ly.backward()
        res = [ly.result() for ly in layers]
        if profile:
            tab = lctx.prof_table()
    finally:
        lctx.prof_enable(False)
        lctx.set_option("gat_bf16", 0)
    for ly in layers:
        ly.close()
    g_d.close()
    return res, tab


def same_results(a, b, what):
    for ra, rb in zip(a, b):
        for k in ra:
            assert torch.equal(bits32(ra[k]), bits32(rb[k])), (what, k)
            assert torch.isfinite(ra[k]).all() and ra[k].abs().max() > 0, (what, k)


def test_layer_bit_for_bit_on_representable_data(lctx):
    assert lctx.get_option("gat_bf16") == 0  # the default
    f0, tab0 = layer_run(lctx, 0, 1, profile=True)
    b, tab1 = layer_run(lctx, 1, 1, profile=True)
    f1, _ = layer_run(lctx, 0, 1)  # on and off again: the fp32 bits are unchanged
    same_results(f0, b, "bf16 against fp32")
    same_results(f0, f1, "fp32 before and after")
    assert "cast_f32_bf16" not in tab0, tab0
    assert tab1["cast_f32_bf16"]["count"] == 2, tab1  # h in forward, grad in backward: the kept copy of h is reused
    assert tab1["gat_fwd_fused"]["count"] == 1 and tab1["gat_bwd_fused"]["count"] == 1, tab1
    with pytest.raises(capi.GaibError):
        lctx.set_option("gat_bf16", 2)


def test_two_layers_interleaved_keep_their_tables(lctx):
    f, _ = layer_run(lctx, 0, 2)
    b, tab = layer_run(lctx, 1, 2, profile=True)
    same_results(f, b, "two layers")
    assert not torch.equal(b[0]["out"], b[1]["out"])  # two different h tables: a shared kept copy would show in layer 0's backward
    assert tab["cast_f32_bf16"]["count"] == 4, tab


# ---- 7. a partitioned GAT graph refuses the option ----------------------------------------------------------------------------
PART_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from graphaibench_amd import layers as L
from util import random_graph
c = L.init(0)
c.set_option("gat_bf16", 1)
rp, ci = random_graph(400, 6, seed=1)
part = L.HostPartition(rp, ci, 0, 1, gat=True)
g = part.make_graph(None)
ld = L.Layer(L.GAT, 1, 400, 32, 32, g, False)
ld.set_heads(4)
ld.write(L.FEAT_IN, torch.randn(400, 32, device="cuda"))
ld.forward(torch.empty(400, 32, device="cuda"))
L.sync()
print("NOT REFUSED")
"""


def test_partitioned_graph_refuses_gat_bf16(tmp_path):
    """a graph with GAT partition structures and gat_bf16 = 1 fails loudly, no silent fp32 path (in a process of its own)"""
    script = tmp_path / "part_gat_bf16.py"
    script.write_text(PART_SCRIPT)
    r = subprocess.run([sys.executable, str(script), str(ROOT)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "NOT REFUSED" not in r.stdout, r.stdout[-1000:] + r.stderr[-1000:]
    assert "gat_bf16" in r.stderr, r.stderr[-1000:]


# ---- 8. the trainer -----------------------------------------------------------------------------------------------------------
# |bf16 - fp32| / fp32 of the final loss: the bar of test_trainer_with_bf16_tables (2 % of the fp32 final loss)
TRAINER_BAR = 0.02


def train(root, dt, epoch_graph):
    exe = ROOT / "bin" / "gpu_train_gat"
    assert exe.exists(), "run graphaibench_amd.build"
    cmd = [str(exe), "cora", "20", "2", "softmax", "64", "0", "0", "0.01", "2", "0", "4", "0"]
    env = dict(os.environ, DATASET_PATH=root, GAIB_GAT_DTYPE=dt, GAIB_GAT_HEADS="8", GAIB_EPOCH_GRAPH=epoch_graph,
               GAIB_EPOCH_LOSSES="1")
    return subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)


@pytest.mark.parametrize("epoch_graph", ["0", "1"])
def test_trainer_with_bf16_gat_tables(tmp_path, epoch_graph):
    root = tb.make_dataset(tmp_path)
    runs, recorded = {}, {}
    for dt in ("fp32", "bf16"):
        r = train(root, dt, epoch_graph)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert f"GAT tables: {dt}" in r.stdout, r.stdout[-2000:]
        recorded[dt] = "recorded as HIP graphs" in r.stderr
        m = re.search(r"epoch_losses ([0-9eE.+\- ]+)", r.stdout + r.stderr)
        losses = [float(v) for v in m.group(1).split()] if m else [float(a) for a in re.findall(r"train_loss ([0-9.]+)", r.stdout)]
        assert len(losses) == 20 and np.isfinite(losses).all(), losses
        runs[dt] = losses
    b, f = runs["bf16"], runs["fp32"]
    print(f"epoch_graph {epoch_graph}: final loss fp32 {f[-1]:.6f} bf16 {b[-1]:.6f} rel {abs(b[-1] - f[-1]) / f[-1]:.3e}")
    assert b[-1] < b[0] * 0.9, b
    if recorded["fp32"]:  # the aggregator's buffers were allocated outside the capture
        assert recorded["bf16"]
    assert abs(b[-1] - f[-1]) <= TRAINER_BAR * f[-1], (b[-1], f[-1])


def test_trainer_refuses_an_unknown_gat_dtype(tmp_path):
    r = train(tb.make_dataset(tmp_path), "other", "0")
    assert r.returncode != 0 and "GAIB_GAT_DTYPE" in r.stderr, r.stdout[-500:] + r.stderr[-500:]
