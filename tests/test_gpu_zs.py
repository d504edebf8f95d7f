"""GPU suite, zero-suppressed tables (gaib_pack_zs / gaib_unpack_zs, gaib_spmm_gemm_zs / gaib_spmm_gemm2_zs): the packed bytes
against a Python restatement of the format, the round trip bit for bit, the packed aggregation bit for bit against
gaib_spmm_gemm(2) on the dense table, the refusals, the GCN / SAGE layers with agg_zs 1 against 0, and the guard.
A packed row holds 46 values per half (even columns, odd columns): a row of 92 values fits when it splits 46 + 46, a row
of 93 never does."""
import numpy as np
import pytest
import torch

from graphaibench_amd import capi, layers as L
from util import random_graph

pytestmark = pytest.mark.gpu

CAP = 46  # values either half (even columns, odd columns) of a packed row holds


def bits32(t):
    return t.contiguous().view(torch.int32)


def pack_reference(table: np.ndarray) -> np.ndarray:
    """the format restated: [rows x 128] uint32 bit patterns -> [rows x 96] uint32"""
    rows = table.shape[0]
    out = np.zeros((rows, 96), np.uint32)
    for r in range(rows):
        even, odd = table[r, 0::2], table[r, 1::2]
        m0 = sum(1 << l for l in range(64) if even[l] != 0)
        m1 = sum(1 << l for l in range(64) if odd[l] != 0)
        out[r, 0], out[r, 1] = m0 & 0xffffffff, m0 >> 32
        out[r, 2], out[r, 3] = m1 & 0xffffffff, m1 >> 32
        ev, od = [v for v in even if v != 0], [v for v in odd if v != 0]
        if len(ev) <= CAP and len(od) <= CAP:  # an over-capacity row keeps only its masks
            out[r, 4:4 + 2 * len(ev):2] = ev
            out[r, 5:5 + 2 * len(od):2] = od
    return out


def row_with(n_values: int, rng, n_even=None) -> np.ndarray:
    """128 bit patterns, exactly n_values of them non-zero (n_even of them in even columns when given)"""
    row = np.zeros(128, np.uint32)
    if n_even is None:
        pos = rng.permutation(128)[:n_values]
    else:
        pos = np.concatenate([2 * rng.permutation(64)[:n_even], 2 * rng.permutation(64)[:n_values - n_even] + 1])
    row[pos] = rng.integers(1, 2 ** 32, n_values, dtype=np.uint32)
    return row


def special_table(rows: int, seed: int) -> np.ndarray:
    """random densities per row, with -0.0, NaN, +-inf, subnormals, all-zero rows, dense rows, rows of exactly 92 values that
    fit (46 + 46) and rows of 93 (47 in one half: over capacity)"""
    rng = np.random.default_rng(seed)
    t = np.zeros((rows, 128), np.uint32)
    specials = np.array([0x80000000, 0x7fc00000, 0xffc00001, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x7fffffff], np.uint32)
    for r in range(rows):
        kind = r % 8
        if kind == 0:
            continue  # all zero
        if kind == 1:
            t[r] = row_with(128, rng)
        elif kind == 2:
            t[r] = row_with(2 * CAP, rng, n_even=CAP)
        elif kind == 3:
            t[r] = row_with(2 * CAP + 1, rng, n_even=CAP + (r // 8) % 2)
        else:
            t[r] = row_with(int(rng.integers(0, 129)), rng)
        if kind >= 4:  # sprinkle the special patterns over values and zeros alike
            pos = rng.integers(0, 128, 6)
            t[r, pos] = specials[rng.integers(0, len(specials), 6)]
    return t


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 63, 257, 1001])
def test_pack_matches_the_format_and_round_trips(ctx, rows):
    t = special_table(rows, seed=rows)
    x = torch.from_numpy(t.view(np.int32)).cuda().view(torch.float32)
    over = torch.zeros(1, dtype=torch.int32, device="cuda")
    zs = ctx.pack_zs(x, overflow=over)
    want = pack_reference(t)
    got = zs.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    n_even, n_odd = (t[:, 0::2] != 0).sum(axis=1), (t[:, 1::2] != 0).sum(axis=1)
    fits = (n_even <= CAP) & (n_odd <= CAP)
    n_over = int((~fits).sum())
    assert int(over.item()) == n_over
    back = ctx.unpack_zs(zs, x)
    assert torch.equal(bits32(back), bits32(x))
    # a row of 46 + 46 values is packed, one with 47 in a half keeps its masks only
    vals = n_even + n_odd
    for r in range(rows):
        assert np.count_nonzero(got[r, 4:]) == (vals[r] if fits[r] else 0), (r, vals[r])
    if rows >= 4:
        assert fits[2] and vals[2] == 92 and not fits[3] and vals[3] == 93 and vals[0] == 0 and vals[1] == 128


def test_pack_refuses_other_widths(ctx):
    for ln in (64, 127, 130, 256):
        x = torch.zeros(8, ln, device="cuda")
        out = torch.empty(8, 96, dtype=torch.int32, device="cuda")
        rc = ctx.lib.gaib_pack_zs(ctx.h, 8, ln, x.data_ptr(), out.data_ptr(), None)
        assert rc == -5, (ln, rc)
        rc = ctx.lib.gaib_unpack_zs(ctx.h, 8, ln, out.data_ptr(), x.data_ptr(), x.data_ptr())
        assert rc == -5, (ln, rc)


# ---- the packed aggregation ---------------------------------------------------------------------------------------------
def csr(nrows, src, dst):
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    key = np.unique(src * nrows + dst)
    rows, cols = key // nrows, (key % nrows).astype(np.uint32)
    rowptr = np.zeros(nrows + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr), cols


def graphs(ctx):
    rp, ci = random_graph(2000, 24, seed=1)  # (12 edges per row and more: below that the dense call streams edges, no packed form)
    yield "random", ctx.graph(rp, ci), 2000
    rp, ci = random_graph(3000, 40, seed=2, power_law=True, hub_deg=2500)  # hubs above the heavy threshold (1024)
    yield "powerlaw_hub", ctx.graph(rp, ci), 3000
    rng = np.random.default_rng(3)
    src = rng.integers(0, 2000, 60000)
    src = src[src % 3 != 0]  # every third row empty
    yield "empty_rows", ctx.graph(*csr(2000, src, rng.integers(0, 2000, len(src)))), 2000
    yield "single_vertex", ctx.graph(np.array([0, 1], np.int64), np.array([0], np.uint32)), 1


def masked_table(n, density, gen, over_mix=False):
    """normal values, a share `density` of them kept (the rest +0.0); over_mix: every fifth row dense, every seventh with 93 values"""
    x = torch.randn(n, 128, device="cuda", generator=gen)
    if density <= 0.0:
        x.zero_()
    elif density < 1.0:
        x = x * (torch.rand(n, 128, device="cuda", generator=gen) < density)
    x = torch.where(x == 0, torch.zeros_like(x), x)  # (no -0.0 from the product: the dense call must see what the packed one does anyway)
    if over_mix:
        dense_rows = torch.arange(n, device="cuda")[0::5]
        x[dense_rows] = torch.randn(len(dense_rows), 128, device="cuda", generator=gen)
        r93 = torch.arange(n, device="cuda")[3::7]
        x[r93] = torch.randn(len(r93), 128, device="cuda", generator=gen)
        x[r93, 93:] = 0.0
    return x.contiguous()


def compare(ctx, g, nc, x, kind, len_out, transW, flags, dual, gen, ew=None):
    nv = g.nv
    zs = ctx.pack_zs(x)
    wshape = (len_out, 128) if transW else (128, len_out)
    W = torch.randn(wshape, device="cuda", generator=gen) * 0.2
    rows2 = torch.randn(nv, 128, device="cuda", generator=gen) if dual else None
    W2 = torch.randn(wshape, device="cuda", generator=gen) * 0.2 if dual else None
    agg0 = torch.randn(nv, 128, device="cuda", generator=gen)
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


def test_spmm_gemm_zs_bit_identical(ctx):
    """every graph x density x weight kind x one / two products; transW, the flags and len_out are drawn independently (seeded),
    and the headline combination -- one product, transW, the aggregate as scratch -- runs on every graph and density"""
    gen = torch.Generator(device="cuda").manual_seed(5)
    rng = np.random.default_rng(17)
    n = 0
    seen = set()
    for name, g, nc in graphs(ctx):
        assert g.ne >= 12 * g.nv or name == "single_vertex", (name, g.ne, g.nv)
        if name == "single_vertex":  # one edge: the dense call streams edges unless told not to
            ctx.set_option("spmm_flat", 0)
        try:
            ew = torch.rand(max(g.ne, 1), device="cuda", generator=gen) + 0.1
            for density in (0.0, 0.25, 0.5, 0.75, 1.0, "mix"):
                x = masked_table(nc, 0.5 if density == "mix" else density, gen, over_mix=density == "mix")
                compare(ctx, g, nc, x, capi.W_GCN, 128, True, dict(agg_scratch=True), False, gen, ew)
                for kind in (capi.W_GCN, capi.W_MEAN_T, capi.W_MEAN, capi.W_EDGE):
                    for dual in (False, True):
                        transW, fl, len_out = bool(rng.integers(2)), int(rng.integers(len(FLAGS))), (128, 64, 16)[int(rng.integers(3))]
                        compare(ctx, g, nc, x, kind, len_out, transW, FLAGS[fl], dual, gen, ew)
                        seen.add((dual, transW, fl))
                        n += 1
        finally:
            ctx.set_option("spmm_flat", -1)
        g.close()
    assert n == 4 * 6 * 4 * 2
    assert len(seen) == 2 * 2 * len(FLAGS), sorted(seen)  # every (products, transW, flags) combination was drawn


def test_special_values_aggregate_alike(ctx):
    """-0.0, inf and NaN in the table: stored, gathered and multiplied like any value (NaN payloads are the hardware's on both sides)"""
    gen = torch.Generator(device="cuda").manual_seed(9)
    rp, ci = random_graph(500, 30, seed=4)
    g = ctx.graph(rp, ci)
    x = masked_table(500, 0.5, gen)
    x[::7, 3] = -0.0
    x[::11, 64] = float("inf")
    x[::13, 127] = float("nan")
    compare(ctx, g, 500, x, capi.W_GCN, 128, True, dict(), False, gen)
    g.close()


def test_refusals(ctx):
    gen = torch.Generator(device="cuda").manual_seed(6)
    rp, ci = random_graph(600, 30, seed=7)
    g = ctx.graph(rp, ci)
    assert g.ne >= 12 * g.nv
    x = masked_table(600, 0.5, gen)
    zs = ctx.pack_zs(x)
    W = torch.randn(128, 128, device="cuda", generator=gen)
    agg, out = torch.empty(600, 128, device="cuda"), torch.empty(600, 128, device="cuda")
    # another width
    x64 = torch.randn(600, 64, device="cuda")
    a64, W64 = torch.empty(600, 64, device="cuda"), torch.randn(64, 128, device="cuda")
    assert ctx.spmm_gemm_zs(g, capi.W_GCN, x64, zs, a64, W64, out) is False
    # 64-bit addressing and the two-kernel route
    # ... and the variants of the dense call that have no packed form: the edge stream, the XCD-affine tile supply
    for key, v, back in (("spmm_addr_mode", 2, 0), ("spmm_fuse", 0, 1), ("spmm_chunked", 1, -1), ("spmm_flat", 1, -1),
                         ("spmm_tile_xcd", 1024, -1)):
        ctx.set_option(key, v)
        try:
            assert ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out) is False, key
        finally:
            ctx.set_option(key, back)
    # an image off its 128-B boundary
    buf = torch.empty(600 * 96 + 8, dtype=torch.int32, device="cuda")
    off = buf[8:].view(600, 96)
    assert ctx.spmm_gemm_zs(g, capi.W_GCN, x, off, agg, W, out) is False
    assert ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out) is True
    g.close()


def test_refuses_graphs_the_dense_call_runs_in_another_variant(ctx):
    """short rows (fewer than 12 edges per row: the dense call takes the edge stream, 20-34 % faster than the row form there):
    GAIB_ERR_UNSUPPORTED for one product, by the packed call and by the route query alike; two products have no edge stream"""
    gen = torch.Generator(device="cuda").manual_seed(8)
    rp, ci = random_graph(800, 5, seed=9)
    g = ctx.graph(rp, ci)
    assert 0 < g.ne < 12 * g.nv
    x = masked_table(800, 0.5, gen)
    zs = ctx.pack_zs(x)
    W = torch.randn(128, 128, device="cuda", generator=gen)
    agg, out, ref = torch.empty(800, 128, device="cuda"), torch.full((800, 128), 7.0, device="cuda"), torch.empty(800, 128, device="cuda")
    lib, p = ctx.lib, lambda t: t.data_ptr()
    assert lib.gaib_spmm_gemm_zs_route(ctx.h, g.h, capi.W_GCN, 128, p(x), p(zs), p(agg), None, 128, p(out)) == -5
    assert lib.gaib_spmm_gemm_zs(ctx.h, g.h, capi.W_GCN, None, 128, p(x), p(zs), p(agg), p(W), 1, 128, p(out), 4) == -5
    assert b"edge stream" in lib.gaib_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    assert lib.gaib_spmm_gemm_zs_route(ctx.h, g.h, capi.W_MEAN_T, 128, p(x), p(zs), p(agg), p(x), 128, p(out)) == 0
    ctx.spmm_gemm(g, capi.W_MEAN_T, x, agg, W, ref, transW=True, rows2=x, W2=W)
    assert ctx.spmm_gemm_zs(g, capi.W_MEAN_T, x, zs, agg, W, out, transW=True, rows2=x, W2=W)
    assert torch.equal(bits32(out), bits32(ref))
    ctx.set_option("spmm_flat", 0)  # told to use the row form, the dense call and the packed one agree again
    try:
        assert lib.gaib_spmm_gemm_zs_route(ctx.h, g.h, capi.W_GCN, 128, p(x), p(zs), p(agg), None, 128, p(out)) == 0
    finally:
        ctx.set_option("spmm_flat", -1)
    g.close()


def test_refuses_row_mapped_graph(ctx):
    rp, ci = random_graph(400, 8, seed=8)
    g = ctx.graph(rp, ci)
    rmap = torch.arange(400, dtype=torch.int32, device="cuda")
    capi._check(ctx.lib.gaib_graph_set_row_map(ctx.h, g.h, rmap.data_ptr(), 400), "gaib_graph_set_row_map")
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = masked_table(400, 0.5, gen)
    zs = ctx.pack_zs(x)
    W = torch.randn(128, 128, device="cuda")
    agg, out = torch.zeros(400, 128, device="cuda"), torch.zeros(400, 128, device="cuda")
    assert ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out) is False
    assert ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out, rows2=x, W2=W) is False
    g.close()


def test_refuses_table_too_large_for_a_descriptor(ctx):
    """a dense table of 4 GB or more has no 32-bit buffer descriptor: refused before anything is launched"""
    nc = (1 << 32) // 512 + 64
    rng = np.random.default_rng(12)
    rp = np.arange(0, 16 * 300 + 1, 16, dtype=np.int64)
    ci = np.sort(rng.integers(0, nc, (300, 16)), axis=1).astype(np.uint32).reshape(-1)
    g = ctx.graph(rp, ci, ncols=nc)
    pos = lambda k: torch.rand(k, device="cuda") + 0.05
    g.set_vertex_norm(pos(300), pos(nc), pos(nc), row_inv_deg=pos(300))
    x = torch.zeros(nc, 128, device="cuda")
    zs = torch.empty(nc, 96, dtype=torch.int32, device="cuda")
    W = torch.randn(128, 128, device="cuda")
    agg, out = torch.zeros(300, 128, device="cuda"), torch.zeros(300, 128, device="cuda")
    assert ctx.spmm_gemm_zs(g, capi.W_MEAN, x, zs, agg, W, out) is False
    del x, zs
    g.close()
    torch.cuda.empty_cache()


# ---- the layers: agg_zs 1 against 0 -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lctx():
    c = L.init(0)
    yield c
    c.set_option("agg_zs", 1)
    c.set_option("agg_bf16", 0)
    c.prof_enable(False)


N_LAYER = 3000


def make_layer(kind, feat_drop=0.0, halo=None, seed=21):
    rp, ci = random_graph(N_LAYER, 40, seed=seed, power_law=True, hub_deg=1500)
    assert len(ci) >= 12 * N_LAYER  # (rows long enough for the row form: the packed route exists)
    g = L.LGraph.from_host(rp, ci, add_selfloop=(kind == L.GCN))
    if halo is not None:
        g.set_halo(halo, lambda n, p: None, lambda n: 0)
        g.set_partition_mode(L.LGraph.PART_SPLIT)
    layer = L.Layer(kind, 1, N_LAYER, 128, 128, g, True, feat_drop=feat_drop)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    layer.write(L.FEAT_IN, torch.randn(N_LAYER, 128, device="cuda", generator=gen))
    out = torch.empty(N_LAYER, 128, device="cuda")
    layer.forward(out)
    L.sync()
    gin = torch.randn(N_LAYER, 128, device="cuda", generator=gen)
    return g, layer, out, gin


def backward(lctx, layer, kind, out, gin):
    """one backward from the same state: (grad_out, weight gradients, the masked grad_in), and whether a pack ran"""
    layer.write(L.GRAD_IN, gin)
    grad_out = torch.zeros(N_LAYER, 128, device="cuda")
    lctx.prof_reset()
    layer.backward(out, grad_out)
    L.sync()
    res = [grad_out, layer.tensor(L.W_NEIGH_GRAD, (128, 128)), layer.tensor(L.GRAD_IN, (N_LAYER, 128))]
    if kind == L.SAGE:
        res.append(layer.tensor(L.W_SELF_GRAD, (128, 128)))
    return res, "pack_zs" in lctx.prof_table()


def same_bits(a, b):
    return all(torch.equal(bits32(x), bits32(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("feat_drop", [0.0, 0.5], ids=["plain", "dropout"])
@pytest.mark.parametrize("kind", [L.GCN, L.SAGE], ids=["gcn", "sage"])
def test_layers_same_bits_with_packed_gradients(lctx, kind, feat_drop):
    g, layer, out, gin = make_layer(kind, feat_drop)
    lctx.prof_enable(True)
    try:
        kept = float((out > 0).float().mean())
        assert 0.3 < kept < 0.7, kept
        lctx.set_option("agg_zs", 0)
        ref, packed0 = backward(lctx, layer, kind, out, gin)
        assert not packed0
        lctx.set_option("agg_zs", 1)
        got, packed1 = backward(lctx, layer, kind, out, gin)
        # (SAGE's two-product backward gathers dense until the packed form is measured faster: aggregators.cpp, ZS_TWO_PRODUCTS)
        assert packed1 == (kind == L.GCN), "GCN packs its gradient, SAGE does not"
        assert lctx.get_option("agg_zs_paused") == 0
        assert same_bits(got, ref)
        # the masked gradient is what the dense layer leaves: zeros exactly where the output was cut
        assert bool(((got[2] == 0) | (out > 0)).all())
    finally:
        lctx.prof_enable(False)
        layer.close()
        g.close()


def test_not_packed_under_bf16_or_with_a_halo(lctx):
    lctx.prof_enable(True)
    try:
        g, layer, out, gin = make_layer(L.GCN)
        lctx.set_option("agg_bf16", 1)
        _, packed = backward(lctx, layer, L.GCN, out, gin)
        lctx.set_option("agg_bf16", 0)
        assert not packed
        layer.close()
        g.close()
        halo = lctx.graph(np.zeros(N_LAYER + 1, np.int64), np.zeros(0, np.uint32), ncols=1)
        g, layer, out, gin = make_layer(L.SAGE, halo=halo)
        _, packed = backward(lctx, layer, L.SAGE, out, gin)
        assert not packed
        layer.close()
        g.close()
    finally:
        lctx.set_option("agg_bf16", 0)
        lctx.prof_enable(False)


def test_guard_stops_and_resumes(lctx):
    """a gradient that keeps about 90 % of its entries (every row over capacity): packing stops within a few steps, resumes
    when the density falls, and the outputs are those of the dense layer throughout"""
    g, layer, out50, gin = make_layer(L.GCN, seed=33)
    gen = torch.Generator(device="cuda").manual_seed(34)
    out90 = (torch.rand(N_LAYER, 128, device="cuda", generator=gen) < 0.9).float()
    lctx.prof_enable(True)
    try:
        lctx.set_option("agg_zs", 0)
        ref90, _ = backward(lctx, layer, L.GCN, out90, gin)
        ref50, _ = backward(lctx, layer, L.GCN, out50, gin)
        lctx.set_option("agg_zs", 1)
        got, packed = backward(lctx, layer, L.GCN, out50, gin)
        assert packed and same_bits(got, ref50) and lctx.get_option("agg_zs_paused") == 0
        paused_at = None
        packs = 0
        for step in range(12):
            got, packed = backward(lctx, layer, L.GCN, out90, gin)
            assert same_bits(got, ref90), step
            packs += int(packed)
            if paused_at is None and lctx.get_option("agg_zs_paused") == 1:
                paused_at = step
        assert paused_at is not None and paused_at <= 3, paused_at
        assert packs <= 4, packs  # (the first steps, then one look at the count every eighth call)
        resumed_at = None
        for step in range(24):
            got, packed = backward(lctx, layer, L.GCN, out50, gin)
            assert same_bits(got, ref50), step
            if resumed_at is None and lctx.get_option("agg_zs_paused") == 0:
                resumed_at = step
        assert resumed_at is not None and resumed_at <= 10, resumed_at
        got, packed = backward(lctx, layer, L.GCN, out50, gin)
        assert packed and same_bits(got, ref50)
    finally:
        lctx.set_option("agg_zs", 1)
        lctx.prof_enable(False)
        layer.close()
        g.close()


def test_guard_is_kept_per_table(lctx):
    """two layers in turn, one keeping about 90 % of its gradient and one about 50 %: the dense one stops packing, the sparse
    one keeps packing, and neither decision leaks into the other"""
    gA, layA, _, ginA = make_layer(L.GCN, seed=41)
    gB, layB, outB, ginB = make_layer(L.GCN, seed=42)
    gen = torch.Generator(device="cuda").manual_seed(43)
    out90 = (torch.rand(N_LAYER, 128, device="cuda", generator=gen) < 0.9).float()
    lctx.prof_enable(True)
    try:
        lctx.set_option("agg_zs", 0)
        refA, _ = backward(lctx, layA, L.GCN, out90, ginA)
        refB, _ = backward(lctx, layB, L.GCN, outB, ginB)
        lctx.set_option("agg_zs", 1)
        packsA = packsB = 0
        for step in range(10):
            got, packed = backward(lctx, layA, L.GCN, out90, ginA)
            assert same_bits(got, refA), step
            packsA += int(packed and step >= 2)
            got, packed = backward(lctx, layB, L.GCN, outB, ginB)
            assert same_bits(got, refB), step
            packsB += int(packed)
        assert packsB == 10, packsB  # the sparse layer packed on every step
        assert packsA <= 1, packsA   # the dense layer stopped after its first steps (one look at the count at most)
        assert lctx.get_option("agg_zs_paused") == 1
    finally:
        lctx.set_option("agg_zs", 1)
        lctx.prof_enable(False)
        layA.close()
        layB.close()
        gA.close()
        gB.close()
