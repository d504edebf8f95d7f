"""The exact method without a GPU (tests/exact.py): the 2^24 bound holds, from the data, for every case of
tests/test_gpu_dense_exact.py and tests/test_gpu_agg_exact.py; on that data an fp32 sum taken in any order or any split of K
equals the int64 sum bit for bit, so the data admits one answer; dense_ref equals an int64 product; the regular graph delivers
its degrees, which make the library's weights exact powers of two, and on it the oracle's fp32 aggregation equals agg_ref64
bit for bit; placed puts an operand where it says."""
import numpy as np
import pytest
import torch

import exact as E
import poison as P
from oracle import binding as orc


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.DENSE_CASES, ids=[E.dense_id(c) for c in E.DENSE_CASES])
def test_dense_bound_holds(case):
    """dense_operands asserts max(|A| . |B| + |C0|) < 2^24 itself; here also against the closed form, and the mask's shares"""
    branch, form, M, N, K, variants = case
    assert form in E.FORMS and len(variants) >= 1 and K <= 342000 and 49 * K + 4096 < E.LIMIT
    ops = E.dense_operands(form, M, N, K, seed=1)
    sa, sb = E.dense_shapes(form, M, N, K)
    assert ops.A.shape == sa and ops.B.shape == sb and ops.C0.shape == (M, N) and ops.A.dtype == ops.B.dtype == ops.C0.dtype == np.float32
    assert np.abs(ops.A).max() <= 7 and np.abs(ops.B).max() <= 7 and np.abs(ops.C0).max() <= 4096
    assert np.array_equal(ops.A, np.rint(ops.A)) and np.array_equal(ops.C0, np.rint(ops.C0))
    if form == "mask":
        assert 0.08 < (ops.mask == 0).mean() < 0.12 and 0.42 < (ops.mask < 0).mean() < 0.48
    else:
        assert ops.mask is None


def test_dense_table_is_complete():
    """no row twice, every form present, every variant a value the dispatch knows"""
    keys = [(f, M, N, K) for _, f, M, N, K, _ in E.DENSE_CASES]
    assert len(set(keys)) == len(keys) and {k[0] for k in keys} == set(E.FORMS)
    known = {0, 2, 10, 11, 12, 13, 28, 29, 30, 31, 33, 34, 35, 37, 38, 39, 41, 50, 61, 62, 64, 66, 67}
    assert {v for c in E.DENSE_CASES for v in c[5]} == known
    with pytest.raises(AssertionError):
        E.assert_bound(np.full((1, 400000), 7, np.float32), np.full((400000, 1), 7, np.float32), np.zeros((1, 1), np.float32))


def agg_case_list():
    G = E.irregular_graph()
    for d in E.SPMM_DIMS:
        for heads in E.SPMM_HEADS[d]:
            yield G, dict(d=d, heads=heads)
    for len_in, len_out in E.GEMM_SHAPES + E.SELF_SHAPES + E.BF16_SHAPES:
        yield G, dict(d=len_in, d_out=len_out)
    for len_in, len_out in E.ZS_SHAPES:
        yield G, dict(d=len_in, d_out=len_out, sparse=0.7)


def test_agg_bounds_hold():
    n = 0
    for G, kw in agg_case_list():
        o = E.agg_operands(G, seed=3, **kw)   # asserts the bound from the data
        assert o.top < E.LIMIT and o.ytop < E.LIMIT
        assert np.abs(o.x).max() <= 3 and set(np.unique(o.ew)) == {1.0, 2.0, 3.0}
        n += 1
    assert n == 10 + len(E.GEMM_SHAPES) + 6
    G = E.irregular_graph()
    assert G.deg.max() <= 2100 and 256 * 3 * (3 * 3 * int(G.deg.max()) + 3) + 8 < E.LIMIT   # the closed form at this graph's longest row
    for loop in (False, True):
        R = E.regular_graph(selfloop=loop)
        kinds = ("gcn",) if loop else ("mean", "mean_t")
        o = E.agg_operands(R, max(E.REGULAR_DIMS), max(E.REGULAR_DIMS), seed=4, kinds=kinds, unit=E.UNIT)
        assert o.ew is None and o.top / E.UNIT < E.LIMIT and o.ytop / E.UNIT < E.LIMIT   # in units of the smallest weight, 1 / 1024


# ---- order independence on the real data --------------------------------------------------------------------------------------------
def sum_f32(terms, order):
    """the fp32 sum of terms [n x c] taken one by one in `order` (rounded to fp32 after every addition)"""
    acc = np.zeros(terms.shape[1], np.float32)
    for i in order:
        acc = (acc + terms[i]).astype(np.float32)
    return acc


def check_any_order(terms, c0, want, what):
    """terms [n x c] fp32, the sum over n: three random orders, and 2, 7 and 64 pieces summed apart and then combined"""
    n = terms.shape[0]
    rng = np.random.default_rng(n)
    assert want.dtype == np.int64
    for r in range(3):
        got = (sum_f32(terms, rng.permutation(n)) + c0).astype(np.float32)
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), f"{what}: order {r}"
    for pieces in (2, 7, 64):
        parts = [sum_f32(terms, idx) for idx in np.array_split(rng.permutation(n), pieces)]
        got = (sum_f32(np.stack(parts), range(pieces)) + c0).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), f"{what}: {pieces} pieces"


@pytest.mark.parametrize("form,M,N,K", [("nn", 33, 65, 129), ("tn", 12, 7, 32768), ("mask", 16, 64, 500)])
def test_dense_sums_do_not_depend_on_the_order(form, M, N, K):
    ops = E.dense_operands(form, M, N, K, seed=1)
    tA, tB = E.FORMS[form]
    A, B = (ops.A.T if tA else ops.A), E.effective_b(ops)
    B = B.T if tB else B
    want = A.astype(np.int64) @ B.astype(np.int64) + ops.C0.astype(np.int64)
    rows = [0, M - 1] if K > 1000 else range(M)
    for i in rows:
        check_any_order(A[i][:, None] * B, ops.C0[i], want[i], f"{form} row {i}")   # [K x N] exact products


def test_a_heavy_rows_sum_does_not_depend_on_the_order():
    G = E.irregular_graph()
    o = E.agg_operands(G, 64, 0, 8, seed=3)
    h = G.hubs[1]
    e = slice(int(G.rp[h]), int(G.rp[h + 1]))
    assert e.stop - e.start > 1024
    terms = np.repeat(o.ew[e], 8, axis=1) * o.x[G.ci[e].astype(np.int64)]
    want = E.agg_ref64(G, "edge", o.x, o.ew, 8)[h]
    assert np.array_equal(want, np.rint(want))
    check_any_order(terms.astype(np.float32), np.zeros(64, np.float32), want.astype(np.int64), "the last hub")


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,M,N,K", [("nn", 257, 130, 1000), ("nt", 33, 65, 129), ("tn", 70, 20, 36), ("mask", 130, 130, 777)])
def test_dense_ref_is_the_int64_product(form, M, N, K):
    ops = E.dense_operands(form, M, N, K, seed=2)
    tA, tB = E.FORMS[form]
    A, B = ops.A.astype(np.int64), E.effective_b(ops).astype(np.int64)
    prod = (A.T if tA else A) @ (B.T if tB else B)
    for accum, relu in ((False, False), (True, True), (False, True)):
        want = prod + (ops.C0.astype(np.int64) if accum else 0)
        want = np.maximum(want, 0) if relu else want
        got = E.dense_ref(ops, accum, relu).numpy()
        assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64))
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got)   # the cast the GPU tests compare against is exact
    if form == "mask":
        assert (E.effective_b(ops)[ops.mask <= 0] == 0).all() and (ops.B[ops.mask <= 0] != 0).any()
    # the guard notices one wrong entry
    prod = E.dense_ref(ops).clone()
    E.check_product(ops, prod)
    prod[M // 2, N // 3] += 1
    with pytest.raises(AssertionError):
        E.check_product(ops, prod)


# ---- graphs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", [False, True])
def test_regular_graph(loop):
    G = E.regular_graph(selfloop=loop)
    E.check_regular(G)
    assert set(np.unique(G.deg)) == set(E.CLASSES)
    assert int((G.deg > 1024).sum()) == 0 and int((G.deg >= 1024).sum()) == E.CLASS_N[1024]
    for deg in E.CLASSES:
        r = np.float32(1) / np.sqrt(np.float32(deg))
        assert np.float32(r) * np.float32(r) * np.float32(deg) == 1 and np.float32(1) / np.float32(deg) * np.float32(deg) == 1
        assert np.frexp(np.float32(r))[0] == 0.5 and np.frexp(np.float32(1) / np.float32(deg))[0] == 0.5   # powers of two


def test_irregular_graph():
    G = E.irregular_graph()
    assert G.hubs == (0, G.nv - 1) and G.nv % 16 != 0
    key = G.rows * G.nv + G.ci.astype(np.int64)
    assert np.all(np.diff(key) > 0) and np.array_equal(key, np.sort(G.ci.astype(np.int64) * G.nv + G.rows))
    for thr, least in ((1024, 2), (100, 3), (8, 100)):
        assert int((G.deg > thr).sum()) >= least


@pytest.mark.parametrize("kind", E.REGULAR_KINDS)
def test_oracle_aggregation_is_exact_on_the_regular_graph(kind):
    G = E.regular_graph(selfloop=kind == "gcn")
    o = E.agg_operands(G, 16, 0, seed=5, kinds=(kind,), unit=E.UNIT)
    g = orc.Graph(G.rp, G.ci)
    got = {"gcn": orc.gcn_aggregate, "mean": orc.sage_aggregate, "mean_t": orc.sage_d_aggregate}[kind](g, o.x)
    want = E.agg_ref64(G, kind, o.x)
    E.assert_dyadic(want)
    assert np.array_equal(got, want.astype(np.float32)) and np.array_equal(got.astype(np.float64), want)


def test_agg_ref64_is_poisons():
    """the CSR product against poison.aggregate64's row-by-row sums: to fp64 rounding on real-valued data, equal on integers"""
    G = P.graph(False)
    x, ew = P.features(G.nv, 16, 1), P.edge_weights(G, 4)
    for kind in P.KINDS:
        assert np.allclose(E.agg_ref64(G, kind, x, ew, 4), P.aggregate64(G, kind, x, ew, 4), rtol=1e-13, atol=1e-13), kind
    o = E.agg_operands(G, 16, 0, 4, seed=6)
    for kind in ("edge", "edge_t"):
        assert np.array_equal(E.agg_ref64(G, kind, o.x, o.ew, 4), P.aggregate64(G, kind, o.x, o.ew, 4)), kind


# ---- placement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1, 2])
def test_placed(off):
    src = np.arange(35, dtype=np.float32).reshape(5, 7)
    for fill in (E.NAN_BITS, E.OUT_BITS):
        v = E.placed(src, off, fill=fill)
        buf = v._base
        assert v.shape == (5, 7) and v.is_contiguous() and np.array_equal(v.numpy(), src)
        assert v.data_ptr() % 16 == 4 * off
        assert buf.numel() == 2 * E.GUARD + off + 35 and v.data_ptr() + 4 * 35 == buf.data_ptr() + 4 * (buf.numel() - E.GUARD)  # it ends at the guard
        assert E.guards_intact(v, off, fill=fill)
        assert bool(torch.isnan(buf[:E.GUARD + off]).all()) == (fill == E.NAN_BITS) and bool(torch.isfinite(buf[-E.GUARD:]).all()) == (fill == E.OUT_BITS)
        v[4, 6] = 1.0
        assert E.guards_intact(v, off, fill=fill)
        buf[E.GUARD + off + 35] = 0.0
        assert not E.guards_intact(v, off, fill=fill)
        buf.view(torch.int32)[E.GUARD + off + 35] = fill
        buf[E.GUARD + off - 1] = 0.0
        assert not E.guards_intact(v, off, fill=fill)
