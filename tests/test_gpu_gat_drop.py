"""GPU suite, the one-sweep GAT forward and backward under attention dropout (gaib_gat_forward_fused_drop /
gaib_gat_backward_fused_drop, layer-library option gat_fused_drop): the exact properties (rate 0 = the undropped calls, the
softmax statistics do not see the mask, replay, launch options), the results against the staged formulas in fp64 with the
library's own mask (gaib_dropout on ones, same seed), the GAT layer with the option on against that expectation and against the
staged layer, the refusals, and the trainer with GAIB_GAT_FUSED_DROP.

Leaky-relu' jumps at a score of 0, where two correct evaluations may take either slope.  The data here keeps every
pre-activation score at least 0.25 - rounding away from 0 (off_zero), and the tests assert 1e-5 of that."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import test_gpu_bf16 as tb  # helpers of the plain bf16 suite (imported as a module: its tests are collected there, not here)
from graphaibench_amd import capi, layers as L
from oracle import binding as orc
from test_gpu_bf16 import lctx  # noqa: F401  (fixture)
from util import LONG_SUM_FLOOR, assert_close, random_graph

pytestmark = pytest.mark.gpu
ROOT = tb.ROOT
bits32, dev, feat = tb.bits32, tb.dev, tb.feat

RATE = 0.3
SCALE = np.float32(1.0) / (np.float32(1.0) - np.float32(RATE))
# "hub": the graph of test_gat_attention_dropout -- its hub row of some 1 800 edges is 29 chunks with a tail; "short": every
# row is shorter than a chunk
GRAPHS = {"hub": dict(n=3000, avg_deg=20, seed=31, power_law=True, hub_deg=1200), "short": dict(n=300, avg_deg=6, seed=2)}
SHAPES = [(32, 1), (32, 8), (64, 1), (64, 8), (64, 16), (128, 1), (128, 8), (128, 16)]  # every G and LH = 1 .. 32 lanes
SEED = 0x5EED0001
NAMES = ("out", "row_stats", "grad_out", "alpha_lgrad", "alpha_rgrad")


@functools.lru_cache(maxsize=None)
def host_graph(name):
    rp, ci = random_graph(**GRAPHS[name])
    g_o = orc.Graph(rp, ci).add_selfloop()
    rows = np.repeat(np.arange(g_o.nv), np.diff(g_o.rowptr))
    return rp, ci, g_o, rows, g_o.colidx.astype(np.int64)


def off_zero(x0, W, al, ar, heads):
    """fp32 x next to x0 such that, with h = x W, every a_l.h_v of a head is an odd multiple of 0.25 and every a_r.h_v an even
    one: each score a_l.h_i + a_r.h_c is an odd multiple of 0.25 (both signs occur), up to the fp32 rounding of x.  The least
    change of each row that does it (2 heads linear conditions on a row of x)."""
    d = W.shape[1]
    dh = d // heads
    A = np.zeros((2 * heads, W.shape[0]))
    for k in range(heads):
        sl = slice(k * dh, (k + 1) * dh)
        A[k], A[heads + k] = W[:, sl] @ al[sl], W[:, sl] @ ar[sl]
    cur = x0.astype(np.float64) @ A.T
    want = np.round(cur * 2) / 2
    want[:, :heads] = np.round((cur[:, :heads] - 0.25) * 2) / 2 + 0.25
    return (x0 + (want - cur) @ np.linalg.solve(A @ A.T, A)).astype(np.float32)


def scores64(h, al, ar, heads, rows, col):
    """the pre-activation scores [ne][heads] in fp64, asserted to stay clear of 0"""
    n, d = h.shape
    dh = d // heads
    h3 = h.astype(np.float64).reshape(n, heads, dh)
    sl_ = (h3 * al.astype(np.float64).reshape(heads, dh)).sum(2)
    sr_ = (h3 * ar.astype(np.float64).reshape(heads, dh)).sum(2)
    t = sl_[rows] + sr_[col]
    assert np.abs(t).min() > 1e-5, np.abs(t).min()
    assert (t > 0).any() and (t < 0).any()
    return t


def expectation(g_o, rows, col, hfeat, al, ar, heads, mask, g_act, relu):
    """forward = the oracle's attention . mask . scale aggregated in fp64; backward = the fp64 formulas of
    tests/test_gpu_layers.py::test_gat_attention_dropout with d(out)/d(p_e) masked and rescaled and the gradient flowing back
    along the dropped attention.  g_act(want) -> the gradient that enters the aggregation's backward."""
    n, d = hfeat.shape
    ne, dh = g_o.ne, d // heads
    _, temp, _, norm = orc.gat_aggregate_mh(g_o, hfeat, al, ar, heads)
    norm, temp = norm.reshape(ne, heads), temp.reshape(ne, heads)
    t64 = scores64(hfeat, al, ar, heads, rows, col)
    assert ((temp > 0) == (t64 > 0)).all()
    p_drop = (norm * mask * SCALE).astype(np.float32)
    want = np.zeros((n, d))
    for k in range(heads):
        sl = slice(k * dh, (k + 1) * dh)
        np.add.at(want[:, sl], rows, p_drop[:, k:k + 1].astype(np.float64) * hfeat[col, sl])
    if relu:
        want = np.maximum(want, 0)
    want = want.astype(np.float32)
    ga = g_act(want).astype(np.float64)
    T = np.zeros((n, d))
    lg, rg = np.zeros(d), np.zeros(d)
    for k in range(heads):
        sl = slice(k * dh, (k + 1) * dh)
        hk = hfeat[:, sl].astype(np.float64)
        p = norm[:, k].astype(np.float64)
        dp = (ga[rows][:, sl] * hk[col]).sum(1) * mask[:, k] * float(SCALE)
        rowdot = np.zeros(n)
        np.add.at(rowdot, rows, p * dp)
        ds = p * (dp - rowdot[rows])
        ge = ds * np.where(temp[:, k] > 0, 1.0, 0.2)
        cs, rs = np.zeros(n), np.zeros(n)
        np.add.at(cs, col, ge)
        np.add.at(rs, rows, ge)
        lg[sl], rg[sl] = rs @ hk, cs @ hk
        np.add.at(T[:, sl], col, p_drop[:, k:k + 1].astype(np.float64) * ga[rows][:, sl])  # out_c += (p m s)_(i->c) grad_i
    return want, T, lg, rg


def library_mask(ctx, ne, heads, seed):
    """the mask gaib_dropout draws over an [ne * heads] array under `seed`"""
    ones = torch.ones(ne * heads, device="cuda")
    m = torch.empty(ne * heads, dtype=torch.uint8, device="cuda")
    ctx.dropout(ones, m, torch.empty_like(ones), RATE, seed)
    ctx.sync()
    m = m.cpu().numpy().reshape(ne, heads)
    # (the rate, within five standard deviations of a binomial share over ne * heads draws)
    assert set(np.unique(m)) <= {0, 1} and abs(1.0 - m.mean() - RATE) < 5 * np.sqrt(RATE * (1 - RATE) / m.size)
    return m


@functools.lru_cache(maxsize=None)
def case(gname, d, heads):
    """host inputs of one (graph, shape): h with its scores off zero, the gradient, the alpha vectors"""
    rp, ci, g_o, rows, col = host_graph(gname)
    rng = np.random.default_rng(1000 * d + heads)
    al, ar = (rng.standard_normal(d) * 0.3).astype(np.float32), (rng.standard_normal(d) * 0.3).astype(np.float32)
    h = off_zero(rng.standard_normal((g_o.nv, d)).astype(np.float32), np.eye(d), al, ar, heads)
    gin = rng.standard_normal((g_o.nv, d)).astype(np.float32)
    return h, gin, al, ar


def run(ctx, g, ins, heads, rate=None, scale=None, seed=SEED, relu=False):
    """forward + backward, outputs pre-filled with 7.0; rate None = the undropped calls"""
    h, gin, al, ar = ins
    n, d = h.shape
    out, stats = torch.full((n, d), 7.0, device="cuda"), torch.full((n, heads, 2), 7.0, device="cuda")
    go, lg, rg = torch.full((n, d), 7.0, device="cuda"), torch.full((d,), 7.0, device="cuda"), torch.full((d,), 7.0, device="cuda")
    if rate is None:
        assert ctx.gat_forward_fused(g, h, al, ar, out, stats, heads=heads, relu=relu)
        assert ctx.gat_backward_fused(g, h, gin, out, al, ar, None, go, lg, rg, heads=heads, row_stats=stats)
    else:
        assert ctx.gat_forward_fused_drop(g, h, al, ar, out, stats, rate, seed, scale=scale, heads=heads, relu=relu)
        assert ctx.gat_backward_fused_drop(g, h, gin, out, al, ar, go, lg, rg, stats, rate, seed, scale=scale, heads=heads)
    res = (out, stats, go, lg, rg)
    for name, t in zip(NAMES, res):
        assert torch.isfinite(t).all() and not bool((t == 7.0).all()), name
    return res


def same_bits(a, b, what, names=NAMES):
    for name, x, y in zip(NAMES, a, b):
        if name in names:
            assert torch.equal(bits32(x), bits32(y)), (what, name, int((bits32(x) != bits32(y)).sum()))


def device_case(ctx, gname, d, heads):
    rp, ci, _, _, _ = host_graph(gname)
    g = ctx.graph(rp, ci.view(np.int32)).add_selfloop()
    return g, tuple(dev(a) for a in case(gname, d, heads))


# ---- 1. exact properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", list(GRAPHS))
@pytest.mark.parametrize("d,heads", SHAPES)
def test_exact_properties(ctx, gname, d, heads):
    g, ins = device_case(ctx, gname, d, heads)
    defaults = dict(gat_fused_unroll=4, gat_chunk_xcd=0)
    try:
        plain = run(ctx, g, ins, heads)
        same_bits(plain, run(ctx, g, ins, heads, rate=0.0, scale=1.0), "rate 0, scale 1 against the undropped calls")
        dropped = run(ctx, g, ins, heads, rate=RATE)
        same_bits(plain, dropped, "the softmax statistics do not see the mask", names=("row_stats",))
        assert not torch.equal(plain[0], dropped[0]) and not torch.equal(plain[2], dropped[2])
        same_bits(dropped, run(ctx, g, ins, heads, rate=RATE), "the same seed again")
        other = run(ctx, g, ins, heads, rate=RATE, seed=SEED + 1)
        assert not torch.equal(other[0], dropped[0])
        for opts in (dict(gat_fused_unroll=8), dict(gat_chunk_xcd=1)):  # (300 rows: 75 workgroups, the XCD walk engages)
            for k, v in {**defaults, **opts}.items():
                ctx.set_option(k, v)
            same_bits(dropped, run(ctx, g, ins, heads, rate=RATE), opts)
    finally:
        for k, v in defaults.items():
            ctx.set_option(k, v)
        g.close()


# ---- 2. against the staged formulas with the library's own mask -----------------------------------------------------------------
@pytest.mark.parametrize("gname", list(GRAPHS))
@pytest.mark.parametrize("d,heads", SHAPES)
def test_against_the_staged_formulas_in_fp64(ctx, gname, d, heads):
    _, _, g_o, rows, col = host_graph(gname)
    h, gin, al, ar = case(gname, d, heads)
    g, ins = device_case(ctx, gname, d, heads)
    try:
        out, _, go, lg, rg = run(ctx, g, ins, heads, rate=RATE)
        mask = library_mask(ctx, g_o.ne, heads, SEED)
        want, T, wlg, wrg = expectation(g_o, rows, col, h, al, ar, heads, mask, lambda _w: gin, relu=False)
        what = f"{gname} {d} x {heads}"
        assert_close(out.cpu().numpy(), want, what + " forward", floor=LONG_SUM_FLOOR)
        assert_close(go.cpu().numpy(), T, what + " grad_out", floor=LONG_SUM_FLOOR)
        assert_close(lg.cpu().numpy(), wlg, what + " alpha_l grad", floor=LONG_SUM_FLOOR)
        assert_close(rg.cpu().numpy(), wrg, what + " alpha_r grad", floor=LONG_SUM_FLOOR)
    finally:
        g.close()


# ---- 3. the layer ---------------------------------------------------------------------------------------------------------------
FIRST_SEED = 0xA77E0000  # GAT_Aggregator's first dropout seed


class DropLayer:
    def __init__(self, g_d, n, din, d, heads, x):
        self.ld = L.Layer(L.GAT, 1, n, din, d, g_d, True, score_drop=RATE)
        if heads > 1:
            self.ld.set_heads(heads)
        self.ld.write(L.FEAT_IN, dev(x))
        self.out = torch.empty(n, d, device="cuda")
        self.grad_out = torch.zeros(n, din, device="cuda")

    def forward(self, phase):
        self.ld.set_phase(phase)
        self.ld.forward(self.out)
        L.sync()
        return self.out.clone()

    def backward(self, fwd_out, gin):
        """backward on the EXPECTED forward output (identical relu masks, as test_gat_attention_dropout does)"""
        self.out.copy_(dev(fwd_out))
        self.ld.write(L.GRAD_IN, dev(gin))
        self.ld.backward(self.out, self.grad_out)
        L.sync()

    def check(self, x, W, T, lg, rg, what):
        din, d = W.shape
        assert_close(self.grad_out.cpu().numpy(), T @ W.T.astype(np.float64), what + " grad_out", floor=LONG_SUM_FLOOR)
        assert_close(self.ld.tensor(L.W_NEIGH_GRAD, (din, d)).cpu().numpy(), x.T.astype(np.float64) @ T, what + " W_grad",
                     floor=LONG_SUM_FLOOR)
        assert_close(self.ld.tensor(L.ALPHA_LGRAD, (d,)).cpu().numpy(), lg, what + " alpha_l grad", floor=LONG_SUM_FLOOR)
        assert_close(self.ld.tensor(L.ALPHA_RGRAD, (d,)).cpu().numpy(), rg, what + " alpha_r grad", floor=LONG_SUM_FLOOR)


@pytest.mark.parametrize("heads", [1, 8])
def test_layer_with_the_option(lctx, heads):
    rp, ci, g_o, rows, col = host_graph("hub")
    n, ne, din, d = g_o.nv, g_o.ne, 48, 64
    W = orc.init_glorot(din, d, 1)
    al, ar = orc.init_glorot(d, 1, 2).ravel(), orc.init_glorot(d, 1, 3).ravel()
    x = off_zero(feat(n, din, 3), W.astype(np.float64), al, ar, heads)
    gin = feat(n, d, 4)
    hfeat = orc.matmul(x, W)
    mask = library_mask(lctx, ne, heads, FIRST_SEED)
    want, T, lg, rg = expectation(g_o, rows, col, hfeat, al, ar, heads, mask, lambda w: np.where(w > 0, gin, 0), relu=True)
    g_d = L.LGraph.from_host(rp, ci, add_selfloop=True)
    assert lctx.get_option("gat_fused_drop") == 0  # the default
    layers = []
    try:
        staged, sweep, fallback = (DropLayer(g_d, n, din, d, heads, x) for _ in range(3))
        layers = [staged, sweep, fallback]
        # option 0: the staged path, as ever; its mask is the one re-drawn above
        test0 = staged.forward(1)
        out0 = staged.forward(0)
        m0 = torch.empty(ne * heads, dtype=torch.uint8, device="cuda")
        capi._check(capi.load().gaib_memcpy_d2d(L.load().gaibl_ctx(), m0.data_ptr(), staged.ld.ptr(L.ATTN_MASKS), ne * heads), "d2d")
        L.sync()
        assert np.array_equal(m0.cpu().numpy().reshape(ne, heads), mask)
        assert_close(out0.cpu().numpy(), want, "staged training forward", floor=LONG_SUM_FLOOR)
        # option 1: the one sweep
        lctx.set_option("gat_fused_drop", 1)
        assert torch.equal(bits32(sweep.forward(1)), bits32(test0))  # a test-phase forward drops nothing
        out1 = sweep.forward(0)
        assert_close(out1.cpu().numpy(), want, "one-sweep training forward", floor=LONG_SUM_FLOOR)
        sweep.backward(want, gin)
        sweep.check(x, W, T, lg, rg, "one sweep")
        assert sweep.ld.ptr(L.ATTN_MASKS) in (0, None) and sweep.ld.ptr(L.NORM_SCORES_DROPPED) in (0, None)
        assert not torch.equal(sweep.forward(0), out1)  # the next seed
        # forward in the sweep, backward not allowed to: the staged pieces on the remembered seed
        outf = fallback.forward(0)
        assert torch.equal(bits32(outf), bits32(out1))
        lctx.set_option("gat_fused_bwd", 0)
        fallback.backward(want, gin)
        fallback.check(x, W, T, lg, rg, "staged fallback")
        assert fallback.ld.ptr(L.ATTN_MASKS) not in (0, None)
    finally:
        lctx.set_option("gat_fused_bwd", -1)
        lctx.set_option("gat_fused_drop", 0)
        for ly in layers:
            ly.ld.close()
        g_d.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ctx):
    rp, ci = random_graph(300, 6, seed=2)
    n = 300
    g = ctx.graph(rp, ci.view(np.int32)).add_selfloop()
    rect = ctx.graph(rp, ci.view(np.int32), ncols=n + 40)

    def attempt(graph, d, heads=4, offset=0, rate=RATE, stats_none=False, rows=n):
        gen = torch.Generator(device="cuda").manual_seed(d)
        flat = torch.randn(rows * d + 8, device="cuda", generator=gen)
        h = flat[offset:offset + rows * d].view(rows, d)
        gin = torch.randn(rows, d, device="cuda", generator=gen)
        al, ar = torch.randn(d, device="cuda", generator=gen), torch.randn(d, device="cuda", generator=gen)
        out, stats = torch.full((n, d), 7.0, device="cuda"), torch.full((n, heads, 2), 7.0, device="cuda")
        go, lg, rg = torch.full((n, d), 7.0, device="cuda"), torch.full((d,), 7.0, device="cuda"), torch.full((d,), 7.0, device="cuda")
        fwd_out = torch.randn(n, d, device="cuda", generator=gen)
        st = torch.rand(n, heads, 2, device="cuda", generator=gen) + 0.5
        if rate >= 1.0 or stats_none:
            if not stats_none:
                with pytest.raises(capi.GaibError):
                    ctx.gat_forward_fused_drop(graph, h, al, ar, out, stats, rate, SEED, scale=1.0, heads=heads)
            with pytest.raises(capi.GaibError):
                ctx.gat_backward_fused_drop(graph, h, gin, fwd_out, al, ar, go, lg, rg, None if stats_none else st, rate, SEED,
                                            scale=1.0, heads=heads)
            f = b = False
        else:
            f = ctx.gat_forward_fused_drop(graph, h, al, ar, out, stats, rate, SEED, heads=heads)
            b = ctx.gat_backward_fused_drop(graph, h, gin, fwd_out, al, ar, go, lg, rg, st, rate, SEED, heads=heads)
        ctx.sync()
        # (forward owns out and row_stats, backward grad_out and the two alpha gradients)
        return f, b, all(bool((t == 7.0).all()) for t in (out, stats)), all(bool((t == 7.0).all()) for t in (go, lg, rg))

    try:
        assert attempt(g, 64) == (True, True, False, False)  # (the accepted call, for contrast)
        assert attempt(g, 48) == (False, False, True, True)
        assert attempt(rect, 64, rows=n + 40) == (False, False, True, True)
        assert attempt(g, 64, offset=1) == (False, False, True, True)  # the table 4 bytes off its alignment
        assert attempt(g, 64, rate=1.0) == (False, False, True, True)
        assert attempt(g, 64, stats_none=True) == (False, False, True, True)
        ctx.set_option("gat_fused_fwd", 0)
        assert attempt(g, 64) == (False, True, True, False)  # forward refused: out and row_stats untouched; backward ran
        ctx.set_option("gat_fused_fwd", -1)
        ctx.set_option("gat_fused_bwd", 0)
        assert attempt(g, 64) == (True, False, False, True)
    finally:
        ctx.set_option("gat_fused_fwd", -1)
        ctx.set_option("gat_fused_bwd", -1)
        g.close()
        rect.close()


# ---- 5. the trainer -------------------------------------------------------------------------------------------------------------
PARITY_BAR = 1e-4   # first epoch: the same weights and the same masks (the project's parity bar)
TRAINER_BAR = 0.02  # final loss: the bar of test_gpu_gat_bf16.py


def train(root, switch):
    exe = ROOT / "bin" / "gpu_train_gat"
    assert exe.exists(), "run graphaibench_amd.build"
    cmd = [str(exe), "cora", "20", "2", "softmax", "64", "0.3", "0", "0.01", "2", "0", "4", "0"]
    env = dict(os.environ, DATASET_PATH=root, GAIB_GAT_HEADS="8", GAIB_GAT_FUSED_DROP=switch, GAIB_EPOCH_LOSSES="1")
    return subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)


def test_trainer_with_the_switch(tmp_path):
    root = tb.make_dataset(tmp_path)
    runs = {}
    for switch, line in (("0", "GAT attention dropout: staged"), ("1", "GAT attention dropout: one sweep")):
        r = train(root, switch)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert r.stdout.count(line) == 1 and r.stdout.count("GAT attention dropout:") == 1, r.stdout[-2000:]
        m = re.search(r"epoch_losses ([0-9eE.+\- ]+)", r.stdout + r.stderr)
        losses = [float(v) for v in m.group(1).split()] if m else [float(a) for a in re.findall(r"train_loss ([0-9.]+)", r.stdout)]
        assert len(losses) == 20 and np.isfinite(losses).all(), losses
        runs[switch] = losses
    s, o = runs["0"], runs["1"]
    print(f"first loss staged {s[0]:.7f} one sweep {o[0]:.7f} rel {abs(o[0] - s[0]) / s[0]:.3e}; "
          f"final {s[-1]:.6f} {o[-1]:.6f} rel {abs(o[-1] - s[-1]) / s[-1]:.3e}")
    assert abs(o[0] - s[0]) <= PARITY_BAR * s[0], (o[0], s[0])
    assert o[-1] < 0.9 * o[0] and s[-1] < 0.9 * s[0], (o, s)
    assert abs(o[-1] - s[-1]) <= TRAINER_BAR * s[-1], (o[-1], s[-1])


def test_trainer_refuses_an_unknown_switch_value(tmp_path):
    r = train(tb.make_dataset(tmp_path), "2")
    assert r.returncode != 0 and "GAIB_GAT_FUSED_DROP=2" in r.stderr, r.stdout[-500:] + r.stderr[-500:]
