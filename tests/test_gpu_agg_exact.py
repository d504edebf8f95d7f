"""GPU suite: the aggregations' heavy rows and the product fused behind them held to EXACT sums (tests/exact.py has the method).

Tables, edge weights and W hold small integers; every output's sum of absolute values is below 2^24 (asserted from the data),
so `agg`, `y = act(agg . op(W))` and the self-term form have one fp32 value each, whatever the order of a hub row's 1500
terms, the heavy-row combine, the chunked form, the edge stream or the MFMA epilogue: the comparison with the fp64 reference
(exact.agg_ref64, and agg_ref64 @ W) is torch.equal, by value.  Graphs: exact.irregular_graph (hubs at the FIRST and the LAST
vertex) with integer edge weights per head (W_EDGE, W_EDGE_T), and exact.regular_graph (degrees 4, 16, 64, 256, 1024: the
library's deg^-1/2 and 1/deg are exact powers of two) for W_GCN, W_MEAN and W_MEAN_T.  spmm_heavy_threshold 1024, 100 and 8
(the regular graph also 1023: a row is heavy with MORE edges than the threshold).  Outputs lie between guards that keep their
bits; x, the edge weights and W come back unchanged."""
import functools

import numpy as np
import pytest
import torch

import exact as E
from graphaibench_amd import capi

pytestmark = pytest.mark.gpu

KIND_ID = {"gcn": capi.W_GCN, "mean": capi.W_MEAN, "mean_t": capi.W_MEAN_T, "edge": capi.W_EDGE, "edge_t": capi.W_EDGE_T}
DEFAULTS = dict(spmm_heavy_threshold=1024, spmm_chunked=-1, spmm_flat=-1, spmm_flat_ring=-1, spmm_hot_cold=-1, spmm_tile_xcd=-1,
                spmm_fuse=1)


@pytest.fixture
def knobs(ctx):
    """every option a test may set goes back to its default afterwards"""
    try:
        yield ctx
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


@pytest.fixture(scope="module")
def graphs(ctx):
    """the device graphs: "irregular", ("regular", self loops)"""
    made = {}

    def get(name, loop=False):
        if (name, loop) not in made:
            G = E.irregular_graph() if name == "irregular" else E.regular_graph(selfloop=loop)
            if name == "regular":
                E.check_regular(G)
            made[name, loop] = ctx.graph(G.rp.copy(), G.ci.view(np.int32).copy())
        return made[name, loop]

    yield get
    for g in made.values():
        g.close()


def set_flat(ctx, flat):
    """0: row by row, 1: the edge stream in batches, 2: the edge stream as a software pipeline"""
    ctx.set_option("spmm_flat", min(flat, 1))
    if flat >= 1:
        ctx.set_option("spmm_flat_ring", flat - 1)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


class Table:
    """an input between NaN guards, with the bits it went in with"""

    def __init__(self, a, dtype=None):
        src = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.bf = dtype == torch.bfloat16
        if self.bf:   # (exact.placed lays out float32: a bf16 table lies between the NaN guard rows of poison.table)
            import poison as P

            self.t = P.table(a, torch.bfloat16)
            assert torch.equal(self.t.float(), src), "the table's integers are not bf16 numbers"
        else:
            self.t = E.placed(src, 0)
        self.before = bits(self.t).clone()

    def unchanged(self):
        return torch.equal(bits(self.t), self.before) and (self.bf or E.guards_intact(self.t, 0))


def output(init, shape):
    """an output between OUT_BITS guards, pre-filled with `init` (a continued partial sum) or NaN"""
    src = torch.full(shape, float("nan"), device="cuda") if init is None else torch.from_numpy(np.ascontiguousarray(init)).cuda()
    return E.placed(src, 0, fill=E.OUT_BITS)


def f32(ref64):
    r = np.asarray(ref64, np.float64)
    out = r.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), r), "the reference is no fp32 number"
    return torch.from_numpy(out).cuda()


def same(got, want, what):
    """by value (-0 equals +0), no tolerance; the output's guards keep their bits"""
    assert E.guards_intact(got, 0, fill=E.OUT_BITS), f"{what}: the guards around the output were written"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} entries differ from the exact sum, first at {i}: "
                             f"{got[i].item()!r} for {want[i].item()!r}; rows {sorted(set(bad[:, 0].tolist()))[:8]}")


def relu64(a, on):
    return np.maximum(a, 0) if on else a


# ---- gaib_spmm with integer edge weights --------------------------------------------------------------------------------------------
SPMM_CASES = [(d, h) for d in E.SPMM_DIMS for h in E.SPMM_HEADS[d]]


@pytest.mark.parametrize("d,heads", SPMM_CASES)
def test_spmm(knobs, graphs, d, heads):
    ctx, G, g = knobs, E.irregular_graph(), graphs("irregular")
    o = E.agg_operands(G, d, 0, heads, seed=d)
    x, ew = Table(o.x), Table(o.ew)
    refs = {kind: E.agg_ref64(G, kind, o.x, o.ew, heads) for kind in ("edge", "edge_t")}
    for thr in E.THRESHOLDS:
        ctx.set_option("spmm_heavy_threshold", thr)
        for kind, ref in refs.items():
            for accumulate, relu, chunked in ((False, False, 0), (True, True, 0), (False, True, 1), (True, False, 1)):
                ctx.set_option("spmm_chunked", chunked)
                what = f"spmm {kind} d {d} heads {heads} threshold {thr} chunked {chunked} accumulate {accumulate} relu {relu}"
                out = output(o.agg0 if accumulate else None, (G.nv, d))
                ctx.spmm(g, KIND_ID[kind], x.t, out, edge_w=ew.t, accumulate=accumulate, relu=relu, heads=heads)
                same(out, f32(relu64(ref + (o.agg0 if accumulate else 0), relu)), what)
        assert ctx.graph_stats(g)["n_heavy"] == int((G.deg > thr).sum())
    assert x.unchanged() and ew.unchanged()


@pytest.mark.parametrize("d", [47, 128])
def test_spmm_two_tables(knobs, graphs, d):
    """column ids from n_first on index the second table; n_first lies inside both hubs' rows and most of the others'.  W_EDGE
    only: two tables are a row class of a partition, which the library aggregates with single-head W_EDGE, never W_EDGE_T."""
    ctx, G, g = knobs, E.irregular_graph(), graphs("irregular")
    nf = 1499
    for h in G.hubs:
        nb = G.ci[G.rp[h]:G.rp[h + 1]]
        assert (nb < nf).sum() > 100 and (nb >= nf).sum() > 100
    o = E.agg_operands(G, d, 0, 1, seed=200 + d)
    x1, x2, ew = Table(o.x[:nf]), Table(o.x[nf:]), Table(o.ew)
    refs = {"edge": E.agg_ref64(G, "edge", o.x, o.ew)}
    out = output(None, (G.nv, d))
    with pytest.raises(capi.GaibError):   # (refused on the host, before any launch)
        ctx.spmm_2t(g, capi.W_EDGE_T, x1.t, x2.t, nf, out, edge_w=ew.t)
    for thr in E.THRESHOLDS:
        ctx.set_option("spmm_heavy_threshold", thr)
        for kind, ref in refs.items():
            for accumulate, relu in ((False, False), (True, True)):
                what = f"spmm_2t {kind} d {d} n_first {nf} threshold {thr} accumulate {accumulate} relu {relu}"
                out = output(o.agg0 if accumulate else None, (G.nv, d))
                ctx.spmm_2t(g, KIND_ID[kind], x1.t, x2.t, nf, out, edge_w=ew.t, accumulate=accumulate, relu=relu)
                same(out, f32(relu64(ref + (o.agg0 if accumulate else 0), relu)), what)
    assert x1.unchanged() and x2.unchanged() and ew.unchanged()


# ---- gaib_spmm_gemm -----------------------------------------------------------------------------------------------------------------
# (transW, relu, agg_scratch, accumulate)
GEMM_FORMS = ((False, False, False, False), (True, True, False, False), (False, True, True, False), (True, False, False, True))


def op_w(W, transW):
    """W as the call takes it: [len_in x len_out], or its transpose stored [len_out x len_in]"""
    return np.ascontiguousarray(W.T) if transW else W


@pytest.mark.parametrize("flat", [0, 1, 2])
@pytest.mark.parametrize("len_in,len_out", E.GEMM_SHAPES)
def test_spmm_gemm(knobs, graphs, len_in, len_out, flat):
    ctx, G, g = knobs, E.irregular_graph(), graphs("irregular")
    o = E.agg_operands(G, len_in, len_out, 1, seed=1000 * len_in + len_out)
    x, ew = Table(o.x), Table(o.ew)
    Ws = {t: Table(op_w(o.W, t)) for t in (False, True)}
    agg64 = E.agg_ref64(G, "edge", o.x, o.ew)
    set_flat(ctx, flat)
    for fuse in (0, 1):
        ctx.set_option("spmm_fuse", fuse)
        for thr in E.THRESHOLDS:
            ctx.set_option("spmm_heavy_threshold", thr)
            for transW, relu, scratch, accumulate in GEMM_FORMS:
                what = (f"spmm_gemm {len_in} -> {len_out} flat {flat} fuse {fuse} threshold {thr} transW {transW} relu {relu} "
                        f"agg_scratch {scratch} accumulate {accumulate}")
                a64 = agg64 + (o.agg0 if accumulate else 0)
                agg, y = output(o.agg0 if accumulate else None, (G.nv, len_in)), output(None, (G.nv, len_out))
                ctx.spmm_gemm(g, capi.W_EDGE, x.t, agg, Ws[transW].t, y, transW=transW, relu=relu, agg_scratch=scratch,
                              edge_w=ew.t, accumulate=accumulate)
                same(y, f32(relu64(a64 @ o.W.astype(np.float64), relu)), what + ": y")
                if scratch:
                    assert E.guards_intact(agg, 0, fill=E.OUT_BITS), what + ": the guards around agg were written"
                else:
                    same(agg, f32(a64), what + ": agg")
    assert x.unchanged() and ew.unchanged() and Ws[False].unchanged() and Ws[True].unchanged()


@pytest.mark.parametrize("len_in,len_out", E.SELF_SHAPES)
def test_spmm_gemm_self_term(knobs, graphs, len_in, len_out):
    """y = act(agg . op(W) + x . op(W_self)) in one store"""
    ctx, G, g = knobs, E.irregular_graph(), graphs("irregular")
    o = E.agg_operands(G, len_in, len_out, 1, seed=300 + len_in)
    x, ew = Table(o.x), Table(o.ew)
    agg64 = E.agg_ref64(G, "edge", o.x, o.ew)
    y64 = agg64 @ o.W.astype(np.float64) + o.x.astype(np.float64) @ o.W_self.astype(np.float64)
    for flat in (0, 1, 2):
        set_flat(ctx, flat)
        for thr in E.THRESHOLDS:
            ctx.set_option("spmm_heavy_threshold", thr)
            for transW, relu in ((False, True), (True, False)):
                what = f"spmm_gemm2 {len_in} -> {len_out} flat {flat} threshold {thr} transW {transW} relu {relu}"
                W, W2 = Table(op_w(o.W, transW)), Table(op_w(o.W_self, transW))
                agg, y = output(None, (G.nv, len_in)), output(None, (G.nv, len_out))
                ctx.spmm_gemm(g, capi.W_EDGE, x.t, agg, W.t, y, transW=transW, relu=relu, edge_w=ew.t, rows2=x.t, W2=W2.t)
                same(y, f32(relu64(y64, relu)), what + ": y")
                same(agg, f32(agg64), what + ": agg")
                assert W.unchanged() and W2.unchanged()
    assert x.unchanged() and ew.unchanged()


@pytest.mark.parametrize("len_in,len_out", E.BF16_SHAPES)
def test_spmm_gemm_bf16(knobs, graphs, len_in, len_out):
    """the bf16 table: its integers are bf16 numbers, so the sums are the fp32 call's"""
    ctx, G, g = knobs, E.irregular_graph(), graphs("irregular")
    o = E.agg_operands(G, len_in, len_out, 1, seed=400 + len_in)
    x, ew = Table(o.x, torch.bfloat16), Table(o.ew)
    agg64 = E.agg_ref64(G, "edge", o.x, o.ew)
    for flat in (0, 1):
        set_flat(ctx, flat)
        for thr in E.THRESHOLDS:
            ctx.set_option("spmm_heavy_threshold", thr)
            for transW, relu in ((False, True), (True, False)):
                what = f"spmm_gemm_bf16 {len_in} -> {len_out} flat {flat} threshold {thr} transW {transW} relu {relu}"
                W = Table(op_w(o.W, transW))
                agg, y = output(None, (G.nv, len_in)), output(None, (G.nv, len_out))
                ctx.spmm_gemm_bf16(g, capi.W_EDGE, x.t, agg, W.t, y, transW=transW, relu=relu, edge_w=ew.t)
                same(y, f32(relu64(agg64 @ o.W.astype(np.float64), relu)), what + ": y")
                same(agg, f32(agg64), what + ": agg")
                assert W.unchanged()
    assert x.unchanged() and ew.unchanged()


@pytest.mark.parametrize("hot_cold", [-1, 1])
@pytest.mark.parametrize("len_in,len_out", E.ZS_SHAPES)
def test_spmm_gemm_zs(knobs, graphs, len_in, len_out, hot_cold):
    """the packed gather: 70 % of the table's entries are zero, every fifth row is dense (over the packed row's capacity); the
    image unpacks to the table bit for bit"""
    ctx, G, g = knobs, E.irregular_graph(), graphs("irregular")
    ctx.set_option("spmm_flat", 0)       # the row form: the edge stream has no packed gather
    ctx.set_option("spmm_tile_xcd", 0)   # nor has the XCD-affine tile supply
    ctx.set_option("spmm_chunked", 0)    # nor have the ordered chunks, which the dense call takes by itself at threshold 8 (a quarter of the edges in heavy rows)
    ctx.set_option("spmm_hot_cold", hot_cold)
    o = E.agg_operands(G, len_in, len_out, 1, seed=500 + len_in, sparse=0.7)
    nz = (o.x[:, :128] != 0)
    over = (nz[:, 0::2].sum(1) > 46) | (nz[:, 1::2].sum(1) > 46)
    assert over.any() and not over.all()
    x, ew = Table(o.x), Table(o.ew)
    pack, unpack = (ctx.pack_zs, ctx.unpack_zs) if len_in == 128 else (ctx.pack_zs_wide, ctx.unpack_zs_wide)
    zs = pack(x.t)
    zs0 = zs.clone()
    assert torch.equal(bits(unpack(zs, x.t)), x.before), "the packed table does not unpack to the table"
    agg64 = E.agg_ref64(G, "edge", o.x, o.ew)
    for thr in E.THRESHOLDS:
        ctx.set_option("spmm_heavy_threshold", thr)
        for transW, relu in ((False, True), (True, False)):
            what = f"spmm_gemm_zs {len_in} -> {len_out} hot_cold {hot_cold} threshold {thr} transW {transW} relu {relu}"
            W = Table(op_w(o.W, transW))
            agg, y = output(None, (G.nv, len_in)), output(None, (G.nv, len_out))
            assert ctx.spmm_gemm_zs(g, capi.W_EDGE, x.t, zs, agg, W.t, y, transW=transW, relu=relu, edge_w=ew.t), what + ": no packed gather"
            same(y, f32(relu64(agg64 @ o.W.astype(np.float64), relu)), what + ": y")
            same(agg, f32(agg64), what + ": agg")
            assert W.unchanged()
    assert x.unchanged() and ew.unchanged() and torch.equal(zs, zs0)


# ---- the regular graph: W_GCN with self loops, W_MEAN, W_MEAN_T ---------------------------------------------------------------------
REGULAR_OUT = {47: 128, 64: 32, 128: 128, 256: 256}   # len_out of the fused product at each table width


@functools.lru_cache(maxsize=None)
def regular_operands(loop):
    """one set of operands per graph at the widest shape; the narrower cases take its leading columns (a subset of the terms:
    the bound holds a fortiori).  The references: agg per kind in fp64, every value an integer number of 2^-10."""
    G = E.regular_graph(selfloop=loop)
    kinds = ("gcn",) if loop else ("mean", "mean_t")
    o = E.agg_operands(G, 256, 256, 1, seed=77 + loop, kinds=kinds, unit=E.UNIT)
    refs = {k: E.agg_ref64(G, k, o.x) for k in kinds}
    for r in refs.values():
        E.assert_dyadic(r)
    return G, o, refs


@pytest.mark.parametrize("d", E.REGULAR_DIMS)
@pytest.mark.parametrize("kind", E.REGULAR_KINDS)
def test_regular_graph(knobs, graphs, kind, d):
    ctx, loop = knobs, kind == "gcn"
    G, o, refs = regular_operands(loop)
    g = graphs("regular", loop)
    d_out = REGULAR_OUT[d]
    xh, Wh = np.ascontiguousarray(o.x[:, :d]), np.ascontiguousarray(o.W[:d, :d_out])
    agg64 = refs[kind][:, :d]
    y64 = agg64 @ Wh.astype(np.float64)
    E.assert_dyadic(y64)
    x, xb, W = Table(xh), Table(xh, torch.bfloat16), Table(Wh)
    want_agg, want_y, want_relu = f32(agg64), f32(y64), f32(relu64(agg64, True))
    for thr in E.REGULAR_THRESHOLDS:
        ctx.set_option("spmm_heavy_threshold", thr)
        what = f"regular graph {kind} d {d} threshold {thr}"
        for relu in (False, True):
            out = output(None, (G.nv, d))
            ctx.spmm(g, KIND_ID[kind], x.t, out, relu=relu)
            same(out, want_relu if relu else want_agg, f"{what}: spmm relu {relu}")
        assert ctx.graph_stats(g)["n_heavy"] == int((G.deg > thr).sum())
        out = output(None, (G.nv, d))
        ctx.spmm_bf16(g, KIND_ID[kind], xb.t, out)
        same(out, want_agg, what + ": spmm_bf16")
        for fuse in (0, 1):
            ctx.set_option("spmm_fuse", fuse)
            agg, y = output(None, (G.nv, d)), output(None, (G.nv, d_out))
            ctx.spmm_gemm(g, KIND_ID[kind], x.t, agg, W.t, y)
            same(y, want_y, f"{what}: spmm_gemm fuse {fuse} y")
            same(agg, want_agg, f"{what}: spmm_gemm fuse {fuse} agg")
        ctx.set_option("spmm_fuse", 1)
    assert x.unchanged() and xb.unchanged() and W.unchanged()
