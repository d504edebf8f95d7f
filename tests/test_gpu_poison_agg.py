"""GPU suite: non-finite values in the feature table (or the edge weights) of an aggregation reach only the outputs that depend on
them.  tests/poison.py has the method and the graph: every call runs on finite inputs and again with +inf written over a poison
set (all of table row 0 -- the dummy row the kernels point idle lanes at --, all of the last row, 18 rows of which one is
adjacent to a hub, columns 0 and len - 1 of five rows); the dependent entries follow from the adjacency on the host; every other
entry keeps the clean run's bits, the dependent ones are +inf (all weights are positive), non-finite after a product with W.
The clean run is held to an fp64 aggregation (assert_close, default floor: the longest row has 331 terms).  Tables are views
into larger allocations between NaN guard rows, outputs are pre-filled with NaN bits and 64 more behind their end.

Covered: gaib_spmm (five weight kinds x six widths x heavy threshold 1024 / 100 x spmm_chunked 0 / 1 x relu, accumulate,
per-head edge weights with the poison in the weights), spmm_bf16 dense and with ld, spmm_2t and spmm_part_bf16 at a table split
inside the graph, spmm_gemm (four shapes x the row form / the edge stream in batches / as a pipeline, self term, relu, transW),
spmm_gemm_bf16, spmm_gemm_zs at 128 and 256 columns (also with spmm_hot_cold 1)."""
import numpy as np
import pytest
import torch

import poison as P
from graphaibench_amd import capi
from util import assert_close

pytestmark = pytest.mark.gpu

KIND_ID = {"gcn": capi.W_GCN, "mean": capi.W_MEAN, "mean_t": capi.W_MEAN_T, "edge": capi.W_EDGE, "edge_t": capi.W_EDGE_T}
DEFAULTS = dict(spmm_heavy_threshold=1024, spmm_chunked=-1, spmm_flat=-1, spmm_flat_ring=-1, spmm_hot_cold=-1, spmm_tile_xcd=-1)
INF = np.float32(np.inf)


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
    """device graphs of the poison graph, one per (self loops, heavy threshold): a graph caches its heavy-row list"""
    made = {}
    for loop in (False, True):
        P.check_graph(P.graph(loop))

    def get(loop, thr=1024):
        if (loop, thr) not in made:
            G = P.graph(loop)
            made[loop, thr] = ctx.graph(G.rp.copy(), G.ci.view(np.int32).copy())
        return made[loop, thr]

    yield get
    for g in made.values():
        g.close()


def poisoned(x, pm):
    xp = x.copy()
    xp[pm] = INF
    return xp


def dependent(G, pm, what, len_out=None):
    """the dependent set of a feature poison, held to both share conditions on the host before the poisoned call runs; len_out:
    also the product's set (every column of a row with a dependent aggregate)"""
    dep = P.dependent(G, pm)
    P.shares(dep, what)
    if len_out is not None:
        P.shares(np.repeat(dep.any(1)[:, None], len_out, 1), what + " out")
    return dep


def relu64(a, on):
    return np.maximum(a, 0) if on else a


# ---- gaib_spmm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", P.SPMM_DIMS)
@pytest.mark.parametrize("kind", P.KINDS)
def test_spmm(knobs, graphs, kind, d):
    ctx, loop = knobs, kind == "gcn"
    G = P.graph(loop)
    x, ew = P.features(G.nv, d, 11 + d), P.edge_weights(G)
    ewd = P.table(ew) if kind in ("edge", "edge_t") else None
    ref = P.aggregate64(G, kind, x, ew)
    masks = {pl: P.poison_mask(G, pl, d) for pl in P.PLACEMENTS}
    deps = {pl: P.dependent(G, m) for pl, m in masks.items()}
    for pl in P.PLACEMENTS:
        P.shares(deps[pl], f"{kind} {d} {pl}")
    for thr in (1024, P.HEAVY):
        ctx.set_option("spmm_heavy_threshold", thr)
        g = graphs(loop, thr)
        if thr == P.HEAVY:
            assert ctx.graph_stats(g)["n_heavy"] == int((G.deg > P.HEAVY).sum()) == 4  # the hubs, the rows of 128 and 129 edges
        for chunked in (0, 1):
            ctx.set_option("spmm_chunked", chunked)
            for relu in (False, True):
                what = f"spmm {kind} d {d} threshold {thr} chunked {chunked} relu {relu}"

                def run(t, tag):
                    out = P.Out(G.nv, d)
                    ctx.spmm(g, KIND_ID[kind], P.table(t), out.t, edge_w=ewd, relu=relu)
                    return out.host(f"{what} {tag}")

                clean = run(x, "clean")
                assert_close(clean, relu64(ref, relu), what)
                for pl in P.PLACEMENTS:
                    P.compare(clean, run(poisoned(x, masks[pl]), pl), deps[pl], "+inf", f"{what} {pl}")


@pytest.mark.parametrize("d", [16, 64, 128, 300])
@pytest.mark.parametrize("kind", P.KINDS)
def test_spmm_accumulate(knobs, graphs, kind, d):
    """the call continues partial sums: finite, positive ones (a row without an edge then reads the same under relu whether the
    kernel stores it again or leaves it), and rows that do not depend on the poison keep the clean run's bits"""
    ctx, loop = knobs, kind == "gcn"
    G = P.graph(loop)
    x, ew = P.features(G.nv, d, 21 + d), P.edge_weights(G)
    c0 = np.abs(P.features(G.nv, d, 22)) + np.float32(0.5)
    ewd = P.table(ew) if kind in ("edge", "edge_t") else None
    ref = c0.astype(np.float64) + P.aggregate64(G, kind, x, ew)
    for thr in (1024, P.HEAVY):
        ctx.set_option("spmm_heavy_threshold", thr)
        g = graphs(loop, thr)
        for chunked, relu in ((0, False), (0, True), (1, True)):
            ctx.set_option("spmm_chunked", chunked)
            what = f"spmm += {kind} d {d} threshold {thr} chunked {chunked} relu {relu}"

            def run(t, tag):
                out = P.Out(G.nv, d, fill=c0)
                ctx.spmm(g, KIND_ID[kind], P.table(t), out.t, edge_w=ewd, accumulate=True, relu=relu)
                return out.host(f"{what} {tag}")

            clean = run(x, "clean")
            assert_close(clean, relu64(ref, relu), what)
            for pl in P.PLACEMENTS:
                pm = P.poison_mask(G, pl, d)
                dep = dependent(G, pm, f"{what} {pl}")
                P.compare(clean, run(poisoned(x, pm), pl), dep, "+inf", f"{what} {pl}")


@pytest.mark.parametrize("heads,d", P.MH_SHAPES)
@pytest.mark.parametrize("kind", ["edge", "edge_t"])
def test_spmm_per_head_weights_poisoned(knobs, graphs, kind, heads, d):
    """ew[e, h] = +inf on the edges of three rows (a light one, the row of 65 edges, a hub) in heads 1 and heads - 1: that row --
    for W_EDGE_T the rows its edges lead to -- in those heads' columns only; the features carry both signs: not finite"""
    ctx = knobs
    G = P.graph(False)
    x, ew = P.features(G.nv, d, 31 + d), P.edge_weights(G, heads)
    rows, hit = P.ew_rows(G), P.ew_heads(heads)
    ewp = ew.copy()
    ewp[np.ix_(np.isin(G.rows, rows), hit)] = INF
    dep = P.dependent_edge_w(G, kind, rows, hit, heads, d)
    P.shares(dep, f"{kind} {heads} {d}")
    ref = P.aggregate64(G, kind, x, ew, heads)
    assert np.array_equal(~np.isfinite(P.aggregate64(G, kind, x, ewp, heads)), dep)
    xd = P.table(x)
    for thr in (1024, P.HEAVY):
        ctx.set_option("spmm_heavy_threshold", thr)
        g = graphs(False, thr)
        for chunked in (0, 1):
            ctx.set_option("spmm_chunked", chunked)
            what = f"spmm {kind} heads {heads} d {d} threshold {thr} chunked {chunked}"

            def run(w, tag):
                out = P.Out(G.nv, d)
                ctx.spmm(g, KIND_ID[kind], xd, out.t, edge_w=P.table(w), heads=heads)
                return out.host(f"{what} {tag}")

            clean = run(ew, "clean")
            assert_close(clean, ref, what)
            P.compare(clean, run(ewp, "poisoned weights"), dep, "nonfinite", what)


# ---- bf16 tables --------------------------------------------------------------------------------------------------------------------
def bf16_round(a):
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize("d", [16, 47, 64, 128, 300])
@pytest.mark.parametrize("kind", ["gcn", "mean", "mean_t", "edge"])
def test_spmm_bf16(knobs, graphs, kind, d):
    """the bf16 table dense and at the gather's own row stride (columns behind d hold +0.0, as gaib_cast_f32_bf16_rows leaves them);
    the poison is bf16's +inf"""
    ctx, loop = knobs, kind == "gcn"
    G = P.graph(loop)
    x, ew = bf16_round(P.features(G.nv, d, 41 + d)), P.edge_weights(G)
    ewd = P.table(ew) if kind == "edge" else None
    ref = P.aggregate64(G, kind, x, ew)
    for thr in (1024, P.HEAVY):
        ctx.set_option("spmm_heavy_threshold", thr)
        g = graphs(loop, thr)
        ld = ctx.bf16_row_stride(g, d)
        assert ld >= d
        for use_ld in (False, True):
            for relu in (False, True):
                what = f"spmm_bf16 {kind} d {d} ld {ld if use_ld else None} threshold {thr} relu {relu}"

                def run(t, tag):
                    if use_ld:
                        wide = np.zeros((G.nv, ld), np.float32)
                        wide[:, :d] = t
                        t = wide
                    out = P.Out(G.nv, d)
                    ctx.spmm_bf16(g, KIND_ID[kind], P.table(t, torch.bfloat16), out.t, edge_w=ewd, relu=relu, ld=ld if use_ld else None)
                    return out.host(f"{what} {tag}")

                clean = run(x, "clean")
                assert_close(clean, relu64(ref, relu), what)
                for pl in P.PLACEMENTS:
                    pm = P.poison_mask(G, pl, d)
                    dep = dependent(G, pm, f"{what} {pl}")
                    P.compare(clean, run(poisoned(x, pm), pl), dep, "+inf", f"{what} {pl}")


# ---- two feature tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [47, 64, 128])
@pytest.mark.parametrize("kind", ["gcn", "mean", "mean_t", "edge"])
@pytest.mark.parametrize("bf", [False, True])
def test_spmm_two_tables(knobs, graphs, bf, kind, d):
    """column ids from n_first on index the second table: +inf in its row 0, in the last row of the first, in both -- each
    a guarded allocation of its own, so a row taken from the wrong table is a NaN guard row or a dependent-set violation"""
    ctx, loop = knobs, kind == "gcn"
    G = P.graph(loop)
    nf = P.n_first(G)
    x, ew = P.features(G.nv, d, 51 + d), P.edge_weights(G)
    if bf:
        x = bf16_round(x)
    ewd = P.table(ew) if kind == "edge" else None
    ref = P.aggregate64(G, kind, x, ew)
    dt = torch.bfloat16 if bf else None
    for thr in (1024, P.HEAVY):
        ctx.set_option("spmm_heavy_threshold", thr)
        g = graphs(loop, thr)
        for relu in (False, True):
            what = f"{'spmm_part_bf16' if bf else 'spmm_2t'} {kind} d {d} n_first {nf} threshold {thr} relu {relu}"

            def run(t, tag):
                out = P.Out(G.nv, d)
                call = ctx.spmm_part_bf16 if bf else ctx.spmm_2t
                call(g, KIND_ID[kind], P.table(t[:nf], dt), P.table(t[nf:], dt), nf, out.t, edge_w=ewd, relu=relu)
                return out.host(f"{what} {tag}")

            clean = run(x, "clean")
            assert_close(clean, relu64(ref, relu), what)
            for pl in ("x2row0", "x1last", "both"):
                pm = P.split_mask(G, pl, d)
                dep = P.dependent(G, pm)
                P.shares(dep, f"{what} {pl}")
                P.compare(clean, run(poisoned(x, pm), pl), dep, "+inf", f"{what} {pl}")


# ---- aggregation with the dense product riding on it ----------------------------------------------------------------------------------
GEMM_FORMS = [("gcn", False, True), ("mean", True, False), ("mean_t", False, False), ("edge", True, True)]  # (kind, transW, relu)


def set_flat(ctx, flat):
    """0: row by row, 1: the edge stream in batches, 2: the edge stream as a software pipeline"""
    ctx.set_option("spmm_flat", min(flat, 1))
    if flat >= 1:
        ctx.set_option("spmm_flat_ring", flat - 1)


def weights(len_in, len_out, transW, seed):
    """finite, both signs, no entry near 0"""
    w = P.features(len_out, len_in, seed) if transW else P.features(len_in, len_out, seed)
    return (np.sign(w) * (np.abs(w) + np.float32(0.25)) * np.float32(0.2)).astype(np.float32)


def gemm_check(clean, dirty, dep_agg, relu, what):
    """agg: +inf exactly at the dependent (row, column) pairs; out: the rows with a dependent column are not finite (+inf or 0
    behind a relu), every other row keeps its bits"""
    P.compare(clean[0], dirty[0], dep_agg, "+inf", what + " agg")
    dep_out = np.repeat(dep_agg.any(1)[:, None], clean[1].shape[1], 1)
    P.compare(clean[1], dirty[1], dep_out, "+inf|0" if relu else "nonfinite", what + " out")


@pytest.mark.parametrize("flat", [0, 1, 2])
@pytest.mark.parametrize("len_in,len_out", P.GEMM_SHAPES)
def test_spmm_gemm(knobs, graphs, len_in, len_out, flat):
    ctx = knobs
    set_flat(ctx, flat)
    for kind, transW, relu in GEMM_FORMS:
        loop = kind == "gcn"
        G = P.graph(loop)
        x, ew = P.features(G.nv, len_in, 61 + len_in), P.edge_weights(G)
        W = weights(len_in, len_out, transW, 62)
        ewd = P.table(ew) if kind == "edge" else None
        agg64 = P.aggregate64(G, kind, x, ew)
        out64 = relu64(agg64 @ (W.T if transW else W).astype(np.float64), relu)
        for thr in (1024, P.HEAVY):
            ctx.set_option("spmm_heavy_threshold", thr)
            g = graphs(loop, thr)
            what = f"spmm_gemm {len_in} -> {len_out} {kind} transW {transW} relu {relu} flat {flat} threshold {thr}"

            def run(t, tag):
                agg, out = P.Out(G.nv, len_in), P.Out(G.nv, len_out)
                ctx.spmm_gemm(g, KIND_ID[kind], P.table(t), agg.t, P.table(W), out.t, transW=transW, relu=relu, edge_w=ewd)
                return agg.host(f"{what} {tag} agg"), out.host(f"{what} {tag} out")

            clean = run(x, "clean")
            assert_close(clean[0], agg64, what + " agg")
            assert_close(clean[1], out64, what + " out")
            for pl in P.PLACEMENTS:
                pm = P.poison_mask(G, pl, len_in)
                dep = dependent(G, pm, f"{what} {pl}", len_out)
                gemm_check(clean, run(poisoned(x, pm), pl), dep, relu, f"{what} {pl}")


@pytest.mark.parametrize("flat", [0, 1, 2])
@pytest.mark.parametrize("len_in,len_out", P.GEMM_SHAPES)
def test_spmm_gemm_self_term(knobs, graphs, len_in, len_out, flat):
    """out = act(agg . op(W) + rows2 . op(W2)): +inf in rows 0, 7 and nv - 1 of rows2 makes exactly those rows of out dependent
    (agg none at all); +inf in the table's `some` rows reaches agg and out as without the self term"""
    ctx = knobs
    set_flat(ctx, flat)
    for kind, transW, relu in GEMM_FORMS[:2]:
        loop = kind == "gcn"
        G = P.graph(loop)
        x, r2 = P.features(G.nv, len_in, 71 + len_in), P.features(G.nv, len_in, 72)
        W, W2 = weights(len_in, len_out, transW, 73), weights(len_in, len_out, transW, 74)
        agg64 = P.aggregate64(G, kind, x)
        op = lambda w: (w.T if transW else w).astype(np.float64)  # noqa: E731
        out64 = relu64(agg64 @ op(W) + r2.astype(np.float64) @ op(W2), relu)
        g = graphs(loop, P.HEAVY)
        ctx.set_option("spmm_heavy_threshold", P.HEAVY)
        what = f"spmm_gemm2 {len_in} -> {len_out} {kind} transW {transW} relu {relu} flat {flat}"

        def run(t, rows2, tag):
            agg, out = P.Out(G.nv, len_in), P.Out(G.nv, len_out)
            ctx.spmm_gemm(g, KIND_ID[kind], P.table(t), agg.t, P.table(W), out.t, transW=transW, relu=relu, rows2=P.table(rows2),
                          W2=P.table(W2))
            return agg.host(f"{what} {tag} agg"), out.host(f"{what} {tag} out")

        clean = run(x, r2, "clean")
        assert_close(clean[0], agg64, what + " agg")
        assert_close(clean[1], out64, what + " out")
        r2p = r2.copy()
        r2p[list(P.ROWS2_POISON)] = INF
        dirty = run(x, r2p, "rows2")
        dep = np.zeros((G.nv, len_out), bool)
        dep[list(P.ROWS2_POISON)] = True
        P.shares(dep, what)
        P.compare(clean[0], dirty[0], np.zeros_like(clean[0], bool), None, what + " rows2: agg")
        P.compare(clean[1], dirty[1], dep, "+inf|0" if relu else "nonfinite", what + " rows2: out")
        pm = P.poison_mask(G, "some", len_in)
        dep = dependent(G, pm, what + " some", len_out)
        gemm_check(clean, run(poisoned(x, pm), r2, "some"), dep, relu, what + " some")


@pytest.mark.parametrize("len_in,len_out", [(128, 128), (64, 48), (256, 128)])
def test_spmm_gemm_bf16(knobs, graphs, len_in, len_out):
    ctx = knobs
    for flat in (0, 1):
        set_flat(ctx, flat)
        for kind, transW, relu in GEMM_FORMS[:2]:
            loop = kind == "gcn"
            G = P.graph(loop)
            x = bf16_round(P.features(G.nv, len_in, 81 + len_in))
            W = weights(len_in, len_out, transW, 82)
            agg64 = P.aggregate64(G, kind, x)
            out64 = relu64(agg64 @ (W.T if transW else W).astype(np.float64), relu)
            g = graphs(loop, P.HEAVY)
            ctx.set_option("spmm_heavy_threshold", P.HEAVY)
            what = f"spmm_gemm_bf16 {len_in} -> {len_out} {kind} transW {transW} relu {relu} flat {flat}"

            def run(t, tag):
                agg, out = P.Out(G.nv, len_in), P.Out(G.nv, len_out)
                ctx.spmm_gemm_bf16(g, KIND_ID[kind], P.table(t, torch.bfloat16), agg.t, P.table(W), out.t, transW=transW, relu=relu)
                return agg.host(f"{what} {tag} agg"), out.host(f"{what} {tag} out")

            clean = run(x, "clean")
            assert_close(clean[0], agg64, what + " agg")
            assert_close(clean[1], out64, what + " out")
            for pl in P.PLACEMENTS:
                pm = P.poison_mask(G, pl, len_in)
                dep = dependent(G, pm, f"{what} {pl}", len_out)
                gemm_check(clean, run(poisoned(x, pm), pl), dep, relu, f"{what} {pl}")


# ---- zero-suppressed tables ---------------------------------------------------------------------------------------------------------
def sparse_table(G, d, seed):
    """a gradient-like table: 30 % of the entries kept; every fifth row and the first of the `some` rows dense (over the packed
    row's capacity of 46 values a half), the second of the `some` rows sparse"""
    rng = np.random.default_rng(seed)
    x = P.features(G.nv, d, seed) * (rng.random((G.nv, d)) < 0.3)
    x = np.where(x == 0, np.float32(0), x).astype(np.float32)
    some = P.some_rows(G.selfloop)
    dense = sorted((set(range(0, G.nv, 5)) | {some[0]}) - {some[1]})
    x[dense] = P.features(G.nv, d, seed + 1)[dense]
    return x


def over_capacity(x):
    """rows of a [n x 128] slab with more than 46 values among its even or among its odd columns"""
    return ((x[:, 0::2] != 0).sum(1) > 46) | ((x[:, 1::2] != 0).sum(1) > 46)


@pytest.mark.parametrize("hot_cold", [-1, 1])
@pytest.mark.parametrize("len_in,len_out", [(128, 128), (256, 128)])
def test_spmm_gemm_zs(knobs, graphs, len_in, len_out, hot_cold):
    """the packed gather (128 columns; 256 as two K-slabs): +inf over the VALUES of the `some` rows, so that a packed row stays a
    packed row -- one of them is over capacity (gathered from the dense table behind the image), as are a fifth of the clean rows"""
    ctx = knobs
    ctx.set_option("spmm_flat", 0)       # the row form: the edge stream has no packed gather
    ctx.set_option("spmm_tile_xcd", 0)   # nor has the XCD-affine tile supply
    ctx.set_option("spmm_hot_cold", hot_cold)
    pack = ctx.pack_zs if len_in == 128 else ctx.pack_zs_wide
    for kind, transW, relu in GEMM_FORMS[:2]:
        loop = kind == "gcn"
        G = P.graph(loop)
        x = sparse_table(G, len_in, 91 + len_in)
        W = weights(len_in, len_out, transW, 92)
        some = list(P.some_rows(loop))
        pm = np.zeros(x.shape, bool)
        pm[some] = x[some] != 0
        xp = poisoned(x, pm)
        over_c, over_p = over_capacity(x[:, :128]), over_capacity(xp[:, :128])
        assert np.array_equal(over_c, over_p) and over_p[some].any() and not over_p[some].all()
        clean_rows = np.setdiff1d(np.arange(G.nv), some)
        assert over_c[clean_rows].any() and not over_c[clean_rows].all()
        dep = P.dependent(G, pm)
        P.shares(dep, f"zs {kind} {len_in}")
        agg64 = P.aggregate64(G, kind, x)
        out64 = relu64(agg64 @ (W.T if transW else W).astype(np.float64), relu)
        for thr in (1024, P.HEAVY):
            ctx.set_option("spmm_heavy_threshold", thr)
            g = graphs(loop, thr)
            what = f"spmm_gemm_zs {len_in} -> {len_out} {kind} transW {transW} relu {relu} threshold {thr} hot_cold {hot_cold}"

            def run(t, tag):
                td = P.table(t)
                zs = pack(td)
                agg, out = P.Out(G.nv, len_in), P.Out(G.nv, len_out)
                assert ctx.spmm_gemm_zs(g, KIND_ID[kind], td, zs, agg.t, P.table(W), out.t, transW=transW, relu=relu), what + ": no packed gather"
                return agg.host(f"{what} {tag} agg"), out.host(f"{what} {tag} out")

            clean = run(x, "clean")
            assert_close(clean[0], agg64, what + " agg")
            assert_close(clean[1], out64, what + " out")
            gemm_check(clean, run(xp, "some"), dep, relu, what)
