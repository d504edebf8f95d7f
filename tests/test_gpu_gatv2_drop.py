"""GPU suite, the one-sweep GATv2 under attention dropout (gaib_gatv2_forward_drop / gaib_gatv2_backward_drop; the layer library's
gat_v2 with gat_fused_drop) against fp64 autograd with the library's own mask (gaib_dropout on ones, same seed) as a dense weight on
the attention; exact properties, refusals, the layer.  Tolerances: util.assert_close defaults, LONG_SUM_FLOOR for a's gradient."""
import numpy as np
import pytest
import torch

from graphaibench_amd import capi, layers as L
from test_gpu_bf16 import lctx  # noqa: F401  (fixture)
from test_gpu_gat_drop import FIRST_SEED, RATE, SCALE, library_mask
from test_gpu_gatv2 import EPS, N, POISON, case, graph, run
from test_gpu_gatv2_wide import case as wide_case
from util import LONG_SUM_FLOOR, assert_close

pytestmark = pytest.mark.gpu

SEED = 0x5EED0002
# narrow; scale 7: rescales, exp underflow; gatv2_wide: two slabs (the head window matters from slab 1 on) and one head
CASES = [(32, 1, 1.5), (32, 8, 1.5), (64, 4, 1.5), (128, 16, 1.5), (64, 4, 7.0), (256, 8, 1.5), (256, 1, 1.5), (512, 1, 1.5)]


def gatv2_drop_64(rp, ci, h, a, heads, mask):
    """(out, h, a) in fp64 with autograd: the scores per edge, scattered into a dense [n][n][heads] array (-inf off the graph) for
    the softmax, which does not see the mask; the weight w [n][n][heads] = mask . scale at (row(e), col(e), k) multiplies p"""
    n, d = h.shape
    row, col = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))), torch.from_numpy(ci.astype(np.int64))
    h, a = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (h, a))
    s_e = (a * torch.nn.functional.leaky_relu(h[row] + h[col], EPS)).reshape(-1, heads, d // heads).sum(-1)
    s = torch.full((n, n, heads), -np.inf, dtype=torch.float64).index_put((row, col), s_e)
    w = torch.zeros(n, n, heads, dtype=torch.float64).index_put((row, col), torch.tensor(mask * float(SCALE), dtype=torch.float64))
    return torch.einsum("ijk,jkc->ikc", torch.softmax(s, 1) * w, h.reshape(n, heads, d // heads)).reshape(n, d), h, a


def run_drop(ctx, gd, h, a, g, heads, rate=RATE, seed=SEED, scale=None, relu=False):
    (hd, ad, gd_), d = (torch.from_numpy(x).cuda() for x in (h, a, g)), h.shape[1]
    out, stats, go, ag = (torch.full(s, POISON, device="cuda") for s in ((N, d), (N, heads, 2), (N, d), (d,)))
    assert ctx.gatv2_forward_drop(gd, hd, ad, out, stats, rate, seed, scale, EPS, heads, relu)
    if not relu:
        assert ctx.gatv2_backward_drop(gd, hd, gd_, out, ad, stats, go, ag, rate, seed, scale, EPS, heads)
    ctx.sync()
    return [t.cpu().numpy() for t in (out, stats, go, ag)]


@pytest.mark.parametrize("d,heads,scale", CASES)
def test_against_fp64(ctx, d, heads, scale):
    rp, ci = graph()
    h, a, g, _ = (wide_case if d > 128 else case)(d, heads, scale)
    gd = ctx.graph(rp, ci)
    try:
        ctx.set_option("gatv2_wide", int(d > 128))
        out, _, go, ag = run_drop(ctx, gd, h, a, g, heads)
        out_relu = run_drop(ctx, gd, h, a, g, heads, relu=True)[0]
        mask = library_mask(ctx, len(ci), heads, SEED)
    finally:
        ctx.set_option("gatv2_wide", 0)
        gd.close()
    want, h64, a64 = gatv2_drop_64(rp, ci, h, a, heads, mask)
    (want * torch.tensor(g, dtype=torch.float64)).sum().backward()
    what, want = f"dropped GATv2 {d} x {heads}, scale {scale}: ", want.detach().numpy()
    assert_close(out, want, what + "out")
    assert_close(out_relu, np.maximum(want, 0.0), what + "relu(out)")
    assert_close(go, h64.grad.numpy(), what + "grad_out")
    assert_close(ag, a64.grad.numpy(), what + "a_grad", floor=LONG_SUM_FLOOR)


@pytest.mark.parametrize("d,heads", [(64, 4), (256, 8), (256, 1)])  # narrow, two slabs, one head
def test_exact_properties(ctx, d, heads):
    h, a, g, _ = (wide_case if d > 128 else case)(d, heads, 1.5)
    gd = ctx.graph(*graph())
    same = lambda x, y: all(np.array_equal(p, q) for p, q in zip(x, y))  # noqa: E731
    try:
        ctx.set_option("gatv2_wide", int(d > 128))
        plain = run(ctx, gd, h, a, g, heads)
        assert same(plain, run_drop(ctx, gd, h, a, g, heads, rate=0.0, scale=1.0)), "rate 0, scale 1 against the undropped calls"
        dropped = run_drop(ctx, gd, h, a, g, heads)
        assert np.array_equal(plain[1], dropped[1]) and not np.array_equal(plain[0], dropped[0]), "the statistics do not see the mask"
        assert same(dropped, run_drop(ctx, gd, h, a, g, heads)), "the same seed again"
        assert not np.array_equal(dropped[0], run_drop(ctx, gd, h, a, g, heads, seed=SEED + 1)[0])
        ctx.set_option("gat_chunk_xcd", 1)  # (some 300 chunks: 77 workgroups, the XCD walk engages)
        assert same(dropped, run_drop(ctx, gd, h, a, g, heads)), "gat_chunk_xcd = 1"
    finally:
        ctx.set_option("gat_chunk_xcd", 0)
        ctx.set_option("gatv2_wide", 0)
        gd.close()


def test_refusals(ctx):
    gd = ctx.graph(*graph())
    directed = ctx.graph(np.array([0, 2, 3, 4], np.int64), np.array([0, 1, 1, 2], np.uint32))  # 0 -> 1 has no reverse
    try:
        for graph_d, n, d, rate, error in ((gd, N, 64, 1.0, "rate"), (gd, N, 64, -0.1, "rate"), (gd, N, 256, RATE, None), (gd, N, 48, RATE, None), (directed, 3, 32, RATE, "symmetric")):
            h, g, fwd, a = (torch.randn(s, device="cuda") for s in ((n, d), (n, d), (n, d), (d,)))
            outs = [torch.full(s, POISON, device="cuda") for s in ((n, d), (n, 1, 2), (n, d), (d,))]
            for call in (lambda: ctx.gatv2_forward_drop(graph_d, h, a, outs[0], outs[1], rate, SEED, 1.0, EPS, 1),
                         lambda: ctx.gatv2_backward_drop(graph_d, h, g, fwd, a, torch.ones(n, 1, 2, device="cuda"), outs[2], outs[3], rate, SEED, 1.0, EPS, 1)):
                if error:
                    with pytest.raises(capi.GaibError, match=error):
                        call()
                else:
                    assert not call()
            ctx.sync()
            assert all(bool((t == POISON).all()) for t in outs), (d, rate)
    finally:
        gd.close()
        directed.close()


@pytest.mark.parametrize("d,heads", [(64, 8), (256, 1)])
def test_through_the_layer(lctx, d, heads):  # noqa: F811
    """GAT_layer 24 -> d with score_drop = RATE under gat_v2 = gat_fused_drop = 1 (gatv2_wide at 256 columns): a test-phase forward
    against a layer without dropout, a training step against fp64 autograd of X -> X W -> dropped GATv2 under the first seed's mask"""
    (rp, ci), din = graph(), 24
    rng = np.random.default_rng(7 + d + heads)
    x, W, g = (rng.standard_normal(s).astype(np.float32) for s in ((N, din), (din, d), (N, d)))
    W *= np.float32(0.3)
    a = (1.5 * rng.standard_normal(d) / np.sqrt(d // heads)).astype(np.float32)
    x64, W64 = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (x, W))
    h64 = x64 @ W64
    want, hleaf, a64 = gatv2_drop_64(rp, ci, h64.detach().numpy(), a, heads, library_mask(lctx, len(ci), heads, FIRST_SEED))
    (want * torch.tensor(g, dtype=torch.float64)).sum().backward()
    h64.backward(hleaf.grad)
    g_d = L.LGraph.from_host(rp, ci, add_selfloop=False)
    options = dict(gat_v2=1, gat_fused_drop=1, gatv2_wide=int(d > 128))
    for k, v in options.items():
        lctx.set_option(k, v)
    ld, plain = layers = [L.Layer(L.GAT, 1, N, din, d, g_d, False, score_drop=sd) for sd in (RATE, 0.0)]
    try:
        for ly in layers:
            ly.set_heads(heads)
            for which, t in ((L.W_NEIGH, W), (L.ALPHA_L, a), (L.FEAT_IN, x), (L.GRAD_IN, g)):
                ly.write(which, torch.from_numpy(t).cuda())
        got, undropped, gx = (torch.full(s, POISON, device="cuda") for s in ((N, d), (N, d), (N, din)))
        plain.forward(undropped)
        ld.set_phase(1)
        ld.forward(got)
        L.sync()
        assert torch.equal(got, undropped)  # a test-phase forward drops nothing
        ld.set_phase(0)
        ld.forward(got)
        ld.backward(got, gx)
        L.sync()
        assert_close(got.cpu().numpy(), want.detach().numpy(), "layer out")
        assert_close(gx.cpu().numpy(), x64.grad.numpy(), "layer input gradient")
        assert_close(ld.tensor(L.W_NEIGH_GRAD, (din, d)).cpu().numpy(), W64.grad.numpy(), "layer weight gradient")
        assert_close(ld.tensor(L.ALPHA_LGRAD, (d,)).cpu().numpy(), a64.grad.numpy(), "layer a gradient", floor=LONG_SUM_FLOOR)
        assert not ld.tensor(L.ALPHA_RGRAD, (d,)).any()  # one vector: the second gradient stays zero
        ld.forward(undropped)
        L.sync()
        assert not torch.equal(got, undropped)  # the next seed
    finally:
        for k in options:
            lctx.set_option(k, 0)
        for ly in layers:
            ly.close()
        g_d.close()
