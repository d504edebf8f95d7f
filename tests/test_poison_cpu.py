"""The poison method without a GPU (tests/poison.py): the graph delivers what it promises, every case keeps the two share
conditions, the dependent masks equal those obtained by brute force from util.dense_adj, and the oracle's own aggregation and
matmul, run clean and poisoned on the CPU, satisfy the method's assertions 1 and 2."""
import numpy as np
import pytest

import poison as P
from oracle import binding as orc
from util import assert_close, dense_adj


@pytest.mark.parametrize("loop", [False, True])
def test_graph_delivers_every_row_length(loop):
    G = P.graph(loop)
    P.check_graph(G)
    assert 590 <= G.nv <= 620 and G.nv % 16 != 0
    for k in P.EXACT:
        assert (G.deg == k + G.loop).any(), k
    heavy = np.nonzero(G.deg > P.HEAVY)[0]
    assert sorted(heavy) == sorted(list(G.hubs) + [G.exact[128], G.exact[129]])  # what spmm_heavy_threshold = 100 makes heavy
    some = P.some_rows(loop)
    a, b = (set(P.neighbours(G, h)) for h in G.hubs)
    assert set(some) & a and not set(some) & b and 0.02 <= len(some) / G.nv <= 0.04
    assert not set(P.quiet_rows(loop)) & (a | b)
    nf = P.n_first(G)
    assert 0 < nf < G.nv and G.deg[nf] > G.loop and G.deg[nf - 1] > G.loop
    assert np.array_equal(P.reverse_edges(G)[P.reverse_edges(G)], np.arange(G.ne))


def test_every_case_keeps_both_shares():
    n = 0
    for what, dep in P.agg_cases():
        P.shares(dep, what)
        n += 1
    for form, tA, tB, M, N, K, variant in P.DENSE_FORMS:
        for side in "MN":
            P.shares(P.dense_dependent(M, N, side), f"{form} {M} {N} {K} {side}")
            n += 1
    assert n > 100
    with pytest.raises(AssertionError):
        P.shares(np.zeros((4, 4), bool))
    with pytest.raises(AssertionError):
        P.shares(np.ones((4, 4), bool))


@pytest.mark.parametrize("loop", [False, True])
def test_dependent_masks_equal_brute_force(loop):
    G = P.graph(loop)
    A = dense_adj(G.rp, G.ci)
    assert np.array_equal(A > 0, P.pattern(G))
    for d in (16, 47):
        for pl in P.PLACEMENTS:
            pm = P.poison_mask(G, pl, d)
            assert np.array_equal(P.dependent(G, pm), (A @ pm.astype(np.float64)) > 0), (pl, d)
    for pl in ("x2row0", "x1last", "both"):
        pm = P.split_mask(G, pl, 8)
        assert np.array_equal(P.dependent(G, pm), (A @ pm.astype(np.float64)) > 0), pl
    # edge-weight poison: the dense matrix of poisoned weights, per head; W_EDGE_T is its transpose
    rows, heads, d = P.ew_rows(G), 4, 16
    hit = np.isin(G.rows, rows)
    Wp = dense_adj(G.rp, G.ci, hit.astype(np.float64))
    for kind, M in (("edge", Wp), ("edge_t", Wp.T)):
        want = np.zeros((G.nv, d), bool)
        for h in P.ew_heads(heads):
            want[:, h * 4:(h + 1) * 4] = (M.sum(1) > 0)[:, None]
        assert np.array_equal(P.dependent_edge_w(G, kind, rows, P.ew_heads(heads), heads, d), want), kind


@pytest.mark.parametrize("kind", P.KINDS)
def test_weights_are_the_oracles(kind):
    """weights64 / aggregate64 restate what the oracle's named aggregators compute"""
    G = P.graph(kind == "gcn")
    g = orc.Graph(G.rp, G.ci)
    x, ew = P.features(G.nv, 16, 1), P.edge_weights(G)
    got = {"gcn": lambda: orc.gcn_aggregate(g, x), "mean": lambda: orc.sage_aggregate(g, x),
           "mean_t": lambda: orc.sage_d_aggregate(g, x), "edge": lambda: orc.spmm_edge(g, ew, x),
           "edge_t": lambda: orc.spmm_edge(g, orc.symmetric_csr_transpose(g, ew), x)}[kind]()
    assert_close(got, P.aggregate64(G, kind, x, ew), kind)


@pytest.mark.parametrize("placement", P.PLACEMENTS)
@pytest.mark.parametrize("kind", P.KINDS)
def test_method_on_the_oracles_aggregation(kind, placement):
    G = P.graph(kind == "gcn")
    g = orc.Graph(G.rp, G.ci)
    d = 16
    x, ew = P.features(G.nv, d, 2), P.edge_weights(G)
    pm = P.poison_mask(G, placement, d)
    dep = P.dependent(G, pm)
    P.shares(dep, f"{kind} {placement}")
    xp = x.copy()
    xp[pm] = np.inf

    def run(t):
        w = {"gcn": None, "mean": None, "mean_t": None, "edge": ew, "edge_t": orc.symmetric_csr_transpose(g, ew)}[kind]
        if kind == "gcn":
            return orc.gcn_aggregate(g, t)
        if kind == "mean":
            return orc.sage_aggregate(g, t)
        if kind == "mean_t":
            return orc.sage_d_aggregate(g, t)
        return orc.spmm_edge(g, w, t)

    clean, dirty = run(x), run(xp)
    P.compare(clean, dirty, dep, "+inf", f"oracle {kind} {placement}")
    assert np.array_equal(np.isposinf(P.aggregate64(G, kind, xp, ew)), dep)
    # the method notices a leak: one independent entry that takes the dummy row's value
    leak = dirty.copy()
    i, c = np.argwhere(~dep)[0]
    leak[i, c] += np.float32(1e-3)
    with pytest.raises(AssertionError):
        P.compare(clean, leak, dep, "+inf")


def test_method_on_edge_weight_poison():
    G = P.graph(False)
    g = orc.Graph(G.rp, G.ci)
    heads, d = 4, 16
    x, ew = P.features(G.nv, d, 3), P.edge_weights(G, heads)
    ewp = ew.copy()
    ewp[np.ix_(np.isin(G.rows, P.ew_rows(G)), P.ew_heads(heads))] = np.inf
    for kind in ("edge", "edge_t"):
        dep = P.dependent_edge_w(G, kind, P.ew_rows(G), P.ew_heads(heads), heads, d)
        P.shares(dep, kind)
        outs = []
        for w in (ew, ewp):
            o = np.empty_like(x)
            for h in range(heads):
                wh = np.ascontiguousarray(w[:, h])
                wh = wh if kind == "edge" else orc.symmetric_csr_transpose(g, wh)
                with np.errstate(invalid="ignore"):
                    o[:, h * 4:(h + 1) * 4] = orc.spmm_edge(g, wh, np.ascontiguousarray(x[:, h * 4:(h + 1) * 4]))
            outs.append(o)
        P.compare(outs[0], outs[1], dep, "nonfinite", kind)
        assert np.array_equal(~np.isfinite(P.aggregate64(G, kind, x, ewp, heads)), dep)


@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 0)])
@pytest.mark.parametrize("side", ["M", "N"])
def test_method_on_the_oracles_matmul(tA, tB, side):
    M, N, K = 33, 65, 129
    rng = np.random.default_rng(5)
    A = rng.standard_normal((K, M) if tA else (M, K)).astype(np.float32)
    B = rng.standard_normal((N, K) if tB else (K, N)).astype(np.float32)
    Ap, Bp = P.dense_poison(A, B, tA, tB, side)
    dep = P.dense_dependent(M, N, side)
    P.shares(dep)
    with np.errstate(invalid="ignore"):
        clean, dirty = orc.matmul(A, B, bool(tA), bool(tB)), orc.matmul(Ap, Bp, bool(tA), bool(tB))
    P.compare(clean, dirty, dep, "nonfinite", f"matmul {tA}{tB} {side}")
    assert_close(clean, (A.T if tA else A).astype(np.float64) @ (B.T if tB else B).astype(np.float64))
