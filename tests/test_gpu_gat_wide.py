"""GPU suite, the one-sweep GAT on multi-head rows wider than 128 columns (context option gat_fused_wide; gaib_gat_fused_slabs):
a row of len = S w columns and heads = S Hs heads runs as S column slabs of the narrow kernels on strided rows.  The contract is
exact: in every slab's columns and heads the wide call's outputs have the BITS of the narrow call at (w, Hs) on contiguous copies
of the column windows, under the same options.  Then the refusals, the GAT layer with the option against the staged layer
(outputs, held device memory, the staged fallback of backward, attention dropout unchanged) and the trainer with GAIB_GAT_WIDE."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import test_gpu_bf16 as tb  # helpers (imported as a module: its tests are collected there, not here)
from graphaibench_amd import capi, layers as L
from test_gpu_bf16 import lctx  # noqa: F401  (fixture)
from util import assert_close, random_graph

pytestmark = pytest.mark.gpu
ROOT = tb.ROOT
bits32, dev = tb.bits32, tb.dev

NV = 333  # not a multiple of 4: the last workgroup of the row kernels has idle waves
ISOLATED = (150, 332)  # no edges at all, not even a self loop: empty rows
V64, V65 = 1, 2  # rows of exactly 64 edges (one full chunk, no tail) and 65 (a one-edge tail)
SHAPES = [(256, 8), (256, 2), (256, 64), (512, 8), (192, 6), (160, 5), (1024, 16)]
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def host_graph():
    """symmetric, sorted rows: vertex 0 adjacent to every vertex that has edges (331 edges: 6 chunks, the reduce kernels' lane
    groups wrap), rows of exactly 64 and 65 edges, ~6 random symmetric pairs per row, self loops on all but the two isolated"""
    rng = np.random.default_rng(11)
    live = np.array([v for v in range(NV) if v not in ISOLATED])
    others = np.array([v for v in live if v not in (0, V64, V65)])
    src, dst = [np.zeros(len(live), np.int64)], [live]  # the hub (its self loop included)
    for v, deg in ((V64, 64), (V65, 65)):  # 0, itself and deg - 2 others
        pick = rng.choice(others, deg - 2, replace=False)
        src.append(np.full(len(pick), v))
        dst.append(pick)
    m = 3 * NV
    src.append(rng.choice(others, m))
    dst.append(rng.choice(others, m))
    src, dst = np.concatenate(src), np.concatenate(dst)
    key = np.unique(np.concatenate([src * NV + dst, dst * NV + src, live * NV + live]))
    rows, cols = key // NV, (key % NV).astype(np.uint32)
    rp = np.zeros(NV + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    rp = np.cumsum(rp)
    deg = np.diff(rp)
    assert deg[0] == NV - 2 > 320 and deg[V64] == 64 and deg[V65] == 65 and all(deg[v] == 0 for v in ISOLATED)
    assert 5 < np.delete(deg, [0, V64, V65] + list(ISOLATED)).mean() < 12
    return rp, cols


@functools.lru_cache(maxsize=None)
def host_case(d):
    rng = np.random.default_rng(500 + d)
    h = (0.5 * rng.standard_normal((NV, d))).astype(np.float32)
    gin = (0.5 * rng.standard_normal((NV, d))).astype(np.float32)
    h[5], h[77] = 0.0, -0.0  # a few rows of +-0.0
    gin[9], gin[77] = -0.0, 0.0
    al, ar = (0.3 * rng.standard_normal(d)).astype(np.float32), (0.3 * rng.standard_normal(d)).astype(np.float32)
    return h, gin, al, ar


@pytest.fixture
def graph(ctx):
    rp, ci = host_graph()
    g = ctx.graph(rp, ci.view(np.int32))
    yield g
    g.close()


@pytest.fixture
def wide(ctx):
    """the option on; every knob a test may turn goes back to its default afterwards"""
    defaults = dict(gat_fused_wide=0, gat_chunk_xcd=0, gat_fused_unroll=4, gat_bwd_pk=0, gat_fused_fwd=-1, gat_fused_bwd=-1)
    assert ctx.get_option("gat_fused_wide") == 0  # ships off
    ctx.set_option("gat_fused_wide", 1)
    yield ctx
    for k, v in defaults.items():
        ctx.set_option(k, v)


def filled(*shape):
    return torch.full(shape, SENTINEL, device="cuda")


def forward(ctx, g, h, al, ar, heads, relu):
    n, d = h.shape
    out, stats = filled(n, d), filled(n, heads, 2)
    ok = ctx.gat_forward_fused(g, h, al, ar, out, stats, heads=heads, relu=relu)
    ctx.sync()
    return ok, out, stats


def backward(ctx, g, h, gin, fwd_out, al, ar, stats, heads, norm=None):
    n, d = h.shape
    go, lg, rg = filled(n, d), filled(d), filled(d)
    ok = ctx.gat_backward_fused(g, h, gin, fwd_out, al, ar, norm, go, lg, rg, heads=heads, row_stats=stats)
    ctx.sync()
    return ok, go, lg, rg


def same(a, b, what):
    assert a.shape == b.shape, what
    assert torch.equal(bits32(a.contiguous()), bits32(b.contiguous())), (what, int((bits32(a.contiguous()) != bits32(b.contiguous())).sum()))


def slabs(d, heads):
    w, S = capi.gat_fused_slabs(d, heads)
    assert S >= 2 and w * S == d and heads % S == 0, (d, heads, w, S)
    return w, S, heads // S


# ---- 1. forward: every slab has the bits of the narrow call on contiguous copies -----------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("d,heads", SHAPES)
def test_forward_slab_identity(wide, graph, d, heads, relu):
    ctx = wide
    w, S, Hs = slabs(d, heads)
    h, _, al, ar = (dev(a) for a in host_case(d))
    ok, out, stats = forward(ctx, graph, h, al, ar, heads, relu)
    assert ok, "the wide call was refused"
    assert torch.isfinite(out).all() and torch.isfinite(stats).all() and not bool((out == SENTINEL).any())
    for v in ISOLATED:  # an empty row: zeros, (no edge yet, 0)
        assert bool((out[v] == 0).all()) and bool((stats[v, :, 1] == 0).all())
    for s in range(S):
        c = slice(s * w, (s + 1) * w)
        okn, out_n, stats_n = forward(ctx, graph, h[:, c].contiguous(), al[c].contiguous(), ar[c].contiguous(), Hs, relu)
        assert okn
        same(out[:, c], out_n, f"out, slab {s}")
        same(stats[:, s * Hs:(s + 1) * Hs], stats_n, f"row_stats, slab {s}")


# ---- 2. backward ------------------------------------------------------------------------------------------------------------------
BWD_CASES = [(d, heads, {}) for d, heads in SHAPES] + [(d, heads, dict(gat_chunk_xcd=1)) for d, heads in SHAPES] + \
    [(d, heads, dict(gat_bwd_pk=1)) for d, heads in SHAPES] + [(192, 6, dict(gat_fused_unroll=8))]


@pytest.mark.parametrize("d,heads,opts", BWD_CASES, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_backward_slab_identity(wide, graph, d, heads, opts):
    ctx = wide
    w, S, Hs = slabs(d, heads)
    h, gin, al, ar = (dev(a) for a in host_case(d))
    ok, out, stats = forward(ctx, graph, h, al, ar, heads, False)
    assert ok
    for k, v in opts.items():
        ctx.set_option(k, v)
    ok, go, lg, rg = backward(ctx, graph, h, gin, out, al, ar, stats, heads)
    assert ok, "the wide call was refused"
    for t in (go, lg, rg):
        assert torch.isfinite(t).all() and not bool((t == SENTINEL).any())
    ctx.set_option("gat_bwd_pk", 0)  # the wide path ignores it: the narrow calls it is held to run WITHOUT the packed-math sweep
    for s in range(S):
        c = slice(s * w, (s + 1) * w)
        cut = lambda t: t[:, c].contiguous()  # noqa: E731
        okn, go_n, lg_n, rg_n = backward(ctx, graph, cut(h), cut(gin), cut(out), al[c].contiguous(), ar[c].contiguous(),
                                         stats[:, s * Hs:(s + 1) * Hs].contiguous(), Hs)
        assert okn
        same(go[:, c], go_n, f"grad_out, slab {s}")
        same(lg[c], lg_n, f"alpha_l gradient, slab {s}")
        same(rg[c], rg_n, f"alpha_r gradient, slab {s}")


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def attempt(ctx, g, d, heads, offset=0, stats_none=False, rows=NV):
    """(forward accepted, backward accepted, forward's outputs untouched, backward's outputs untouched)"""
    gen = torch.Generator(device="cuda").manual_seed(d + heads)
    flat = torch.randn(rows * d + 8, device="cuda", generator=gen)
    h = flat[offset:offset + rows * d].view(rows, d)
    gin, fwd_out = torch.randn(rows, d, device="cuda", generator=gen), torch.randn(NV, d, device="cuda", generator=gen)
    al, ar = torch.randn(d, device="cuda", generator=gen), torch.randn(d, device="cuda", generator=gen)
    st = torch.rand(NV, heads, 2, device="cuda", generator=gen) + 0.5
    out, stats = filled(NV, d), filled(NV, heads, 2)
    go, lg, rg = filled(NV, d), filled(d), filled(d)
    f = ctx.gat_forward_fused(g, h, al, ar, out, stats, heads=heads)
    norm = torch.rand(g.ne, heads, device="cuda", generator=gen) if stats_none else None
    b = ctx.gat_backward_fused(g, h, gin, fwd_out, al, ar, norm, go, lg, rg, heads=heads, row_stats=None if stats_none else st)
    ctx.sync()
    untouched = lambda ts: all(bool((t == SENTINEL).all()) for t in ts)  # noqa: E731
    return f, b, untouched((out, stats)), untouched((go, lg, rg))


def test_refusals_leave_the_outputs_untouched(ctx, graph):
    rp, ci = host_graph()
    refused = (False, False, True, True)
    assert ctx.get_option("gat_fused_wide") == 0
    for d, heads in SHAPES:  # option 0: what these shapes always returned
        assert attempt(ctx, graph, d, heads) == refused, (d, heads)
    rect = ctx.graph(rp, ci.view(np.int32), ncols=NV + 40)
    try:
        ctx.set_option("gat_fused_wide", 1)
        assert attempt(ctx, graph, 256, 8) == (True, True, False, False)  # (the accepted call, for contrast)
        assert attempt(ctx, graph, 256, 1) == refused  # a single head wider than 128 columns
        assert attempt(ctx, graph, 200, 8) == refused  # no slab width divides it
        assert attempt(ctx, graph, 256, 8, offset=1) == refused  # the table 4 bytes off its alignment
        # backward without row statistics: refused as the narrow call refuses the shape (forward is not concerned)
        assert attempt(ctx, graph, 256, 8, stats_none=True) == (True, False, False, True)
        assert attempt(ctx, rect, 256, 8, rows=NV + 40) == refused  # a rectangular graph
        ctx.set_option("gat_fused_fwd", 0)
        assert attempt(ctx, graph, 256, 8) == (False, True, True, False)
        ctx.set_option("gat_fused_fwd", -1)
        ctx.set_option("gat_fused_bwd", 0)
        assert attempt(ctx, graph, 256, 8) == (True, False, False, True)
    finally:
        for k, v in dict(gat_fused_wide=0, gat_fused_fwd=-1, gat_fused_bwd=-1).items():
            ctx.set_option(k, v)
        rect.close()


# ---- 4. the layer -----------------------------------------------------------------------------------------------------------------
DIN, DOUT, HEADS = 48, 256, 8


class WideLayer:
    def __init__(self, g_d, n, x, score_drop=0.0):
        self.ld = L.Layer(L.GAT, 1, n, DIN, DOUT, g_d, True, score_drop=score_drop)
        self.ld.set_heads(HEADS)
        self.ld.write(L.FEAT_IN, x)
        self.out = torch.empty(n, DOUT, device="cuda")
        self.grad_out = torch.zeros(n, DIN, device="cuda")

    def forward(self):
        self.ld.forward(self.out)
        L.sync()
        return self.out.clone()

    def backward(self, fwd_out, gin):
        """backward on a GIVEN forward output: identical relu masks in the layers that are compared"""
        self.out.copy_(fwd_out)
        self.ld.write(L.GRAD_IN, gin)
        self.ld.backward(self.out, self.grad_out)
        L.sync()
        return self.grad_out.clone(), self.ld.tensor(L.W_NEIGH_GRAD, (DIN, DOUT))

    def holds_edge_arrays(self):
        return self.ld.ptr(L.NORM_SCORES_GRAD) not in (0, None)


def test_layer_with_the_option_against_the_staged_layer(lctx):
    rp, ci = host_graph()
    rng = np.random.default_rng(21)
    x, gin = dev(rng.standard_normal((NV, DIN)).astype(np.float32)), dev(rng.standard_normal((NV, DOUT)).astype(np.float32))
    g_d = L.LGraph.from_host(rp, ci, add_selfloop=False)  # (the self loops are in the graph)
    made = []

    def layer(**kw):
        made.append(WideLayer(g_d, NV, x, **kw))
        return made[-1]

    def close(a, b, what):
        assert_close(a.cpu().numpy(), b.cpu().numpy(), what)

    assert lctx.get_option("gat_fused_wide") == 0
    try:
        staged, staged_drop = layer(), layer(score_drop=0.3)
        out0 = staged.forward()
        go0, wg0 = staged.backward(out0, gin)
        outd0 = staged_drop.forward()
        god0, wgd0 = staged_drop.backward(outd0, gin)
        assert staged.holds_edge_arrays()
        lctx.set_option("gat_fused_wide", 1)
        sweep, fallback, drop = layer(), layer(), layer(score_drop=0.3)
        out1 = sweep.forward()
        close(out1, out0, "feat_out")
        go1, wg1 = sweep.backward(out0, gin)
        close(go1, go0, "grad_out")
        close(wg1, wg0, "W_neigh_grad")
        assert not sweep.holds_edge_arrays()  # no [ne][heads] array was allocated on the way
        # forward in the sweep, backward not allowed to: the staged pieces from the full-width row statistics
        same(fallback.forward(), out1, "the same forward")
        lctx.set_option("gat_fused_bwd", 0)
        go2, wg2 = fallback.backward(out0, gin)
        lctx.set_option("gat_fused_bwd", -1)
        close(go2, go0, "grad_out, staged fallback")
        close(wg2, wg0, "W_neigh_grad, staged fallback")
        assert fallback.holds_edge_arrays()
        # attention dropout stays staged at these widths: the bits of the option-0 layer
        same(drop.forward(), outd0, "feat_out under attention dropout")
        god1, wgd1 = drop.backward(outd0, gin)
        same(god1, god0, "grad_out under attention dropout")
        same(wgd1, wgd0, "W_neigh_grad under attention dropout")
    finally:
        lctx.set_option("gat_fused_bwd", -1)
        lctx.set_option("gat_fused_wide", 0)
        for ly in made:
            ly.ld.close()
        g_d.close()


def test_layer_holds_less_device_memory_with_the_option(lctx):
    """held after construction and one step (read as tests/test_gpu_lifecycle.py reads free memory): lower with the option by
    at least one [ne][heads] fp32 array -- the staged path holds three of them and a workspace of two more"""
    n = 40_000
    rp, ci = random_graph(n, 24, seed=5, power_law=True, hub_deg=2000)
    x, gin = torch.randn(n, DIN, device="cuda"), torch.randn(n, DOUT, device="cuda")

    def free_bytes():
        L.sync()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def held(option):
        lctx.set_option("gat_fused_wide", option)
        before = free_bytes()
        g_d = L.LGraph.from_host(rp, ci, add_selfloop=True)
        ly = WideLayer(g_d, n, x)
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
    array = ne * HEADS * 4
    print(f"held with the option {h1 / 2**20:.1f} MiB, without {h0 / 2**20:.1f} MiB, one [ne][heads] array {array / 2**20:.1f} MiB")
    assert array > 16 << 20  # (far above the allocator's granularity)
    assert h0 - h1 >= array, (h0, h1, array)


# ---- 5. the trainer ---------------------------------------------------------------------------------------------------------------
PARITY_BAR = 1e-4   # first epoch: the same weights (the trainer tests' parity bar, tests/test_gpu_gat_drop.py)
TRAINER_BAR = 0.02  # final loss (tests/test_gpu_gat_bf16.py)
LINE = "GAT wide rows: one sweep, 2 slabs of 128"


def train(root, switch):
    exe = ROOT / "bin" / "gpu_train_gat"
    assert exe.exists(), "run graphaibench_amd.build"
    cmd = [str(exe), "cora", "10", "2", "softmax", "256", "0", "0", "0.01", "2", "0", "4", "0"]
    env = dict(os.environ, DATASET_PATH=root, GAIB_GAT_HEADS="8", GAIB_EPOCH_LOSSES="1")
    env.pop("GAIB_GAT_WIDE", None)
    if switch is not None:
        env["GAIB_GAT_WIDE"] = switch
    return subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)


def losses_of(r):
    m = re.search(r"epoch_losses ([0-9eE.+\- ]+)", r.stdout + r.stderr)
    assert m, r.stdout[-2000:] + r.stderr[-2000:]
    return [float(v) for v in m.group(1).split()]


def untimed(text):
    """the output lines without those that carry a time or a rate, which differs from run to run (the epoch lines among them: the losses
    are compared at full precision through the epoch_losses line)"""
    return [ln for ln in text.splitlines() if not any(k in ln for k in ("time", "seconds", "Throughput", "edges/s"))]


def test_trainer_with_the_switch(tmp_path):
    root = tb.make_dataset(tmp_path)
    runs = {}
    for switch in (None, "0", "1"):
        r = train(root, switch)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert r.stdout.count("GAT wide rows:") == (1 if switch == "1" else 0), r.stdout[-2000:]
        losses = losses_of(r)
        assert len(losses) == 10 and np.isfinite(losses).all(), losses
        runs[switch] = (losses, r.stdout)
    assert runs["1"][1].count(LINE) == 1, runs["1"][1][-2000:]
    # without the variable, and with it at 0: no call and no output line changes
    assert runs[None][0] == runs["0"][0]
    assert untimed(runs[None][1]) == untimed(runs["0"][1])
    measured = lambda ln: ln.startswith("[gaib prof] epoch_") or ln == LINE  # noqa: E731
    assert [ln for ln in untimed(runs["1"][1]) if not measured(ln)] == [ln for ln in untimed(runs["0"][1]) if not measured(ln)]
    s, o = runs["0"][0], runs["1"][0]
    print(f"first loss staged {s[0]:.7f} one sweep {o[0]:.7f} rel {abs(o[0] - s[0]) / s[0]:.3e}; "
          f"final {s[-1]:.6f} {o[-1]:.6f} rel {abs(o[-1] - s[-1]) / s[-1]:.3e}")
    assert abs(o[0] - s[0]) <= PARITY_BAR * s[0], (o[0], s[0])
    assert o[-1] < 0.9 * o[0] and s[-1] < 0.9 * s[0], (o, s)
    assert abs(o[-1] - s[-1]) <= TRAINER_BAR * s[-1], (o[-1], s[-1])


def test_trainer_refuses_an_unknown_switch_value(tmp_path):
    r = train(tb.make_dataset(tmp_path), "2")
    assert r.returncode != 0 and "GAIB_GAT_WIDE=2" in r.stderr, r.stdout[-500:] + r.stderr[-500:]
