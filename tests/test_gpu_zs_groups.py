"""GPU suite, the packed gather's groups (spmm_core.h: zs_accumulate_group): a packed row is expanded four rows at a time with ONE
branch per group for rows over capacity, in the full batches of 16 and in the tail pieces (8 / 4 / 2 / 1) alike.  One hand-built
graph -- every tail composition, whole batches, the 64-edge chunk boundary, two rows on the heavy kernel -- and masked tables
that put over-capacity rows at chosen places: gaib_spmm_gemm_zs against gaib_spmm_gemm on the dense table, bit for bit in
`out` and `agg`.  Where every over-capacity gather falls (slot of a full batch, slot of a tail piece) is computed on the CPU
from the CSR and the table, and every slot has to be hit before the GPU is used."""
import numpy as np
import pytest
import torch

from graphaibench_amd import capi

pytestmark = pytest.mark.gpu

CAP = 46       # values either half (even columns, odd columns) of a packed row holds
U = 16         # gathers of a full batch (spmm_gemm_zs.hip)
HEAVY = 1024   # rows with more edges run on the heavy kernel: 16 waves, wave w takes the 64-edge chunks w, w + 16, ..
NV = 1536
DEGREES = [0, 1, 2, 3, 4, 7, 8, 9, 12, 15, 16, 17, 24, 31, 32, 33, 47, 48, 63, 64, 65, 80, 127, 128, 129]
HEAVY_ROWS = {700: 1025, 1400: 1300}
TAIL_SLOTS = {(p, u) for p in (8, 4, 2, 1) for u in range(p)}


def bits32(t):
    return t.contiguous().view(torch.int32)


def build_graph():
    rng = np.random.default_rng(101)
    deg = np.array([HEAVY_ROWS.get(r, DEGREES[r % len(DEGREES)]) for r in range(NV)], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.permutation(NV)[:d]) for d in deg]).astype(np.uint32)
    return rowptr, col


def chunks(rowptr):
    """(first edge, edges) of every 64-edge chunk a wave walks: one wave per light row, 16 waves dealing a heavy row's chunks"""
    for r in range(len(rowptr) - 1):
        e0, e1 = int(rowptr[r]), int(rowptr[r + 1])
        for base in range(e0, e1, 64):  # (a heavy row's chunks are the same 64-edge pieces, dealt to its waves)
            yield base, min(64, e1 - base)


def slots_hit(rowptr, col, over_rows):
    """full-batch slots 0..15 and tail slots (piece, position) at which a gather of an over-capacity table row falls"""
    full, tail = set(), set()
    for base, n in chunks(rowptr):
        nfull = n - n % U
        for k in range(n):
            if not over_rows[col[base + k]]:
                continue
            if k < nfull:
                full.add(k % U)
            else:
                pos, r = k - nfull, n % U
                for p in (8, 4, 2, 1):  # the tail's power-of-two pieces, in CSR order
                    if r & p:
                        if pos < p:
                            tail.add((p, pos))
                            break
                        pos -= p
    return full, tail


def half_counts(t):
    return (t[:, 0::2] != 0).sum(axis=1), (t[:, 1::2] != 0).sum(axis=1)


def row_with(rng, n_even, n_odd):
    """128 normal values, exactly n_even kept in the even columns and n_odd in the odd ones (the rest +0.0)"""
    row = np.zeros(128, np.float32)
    pos = np.concatenate([2 * rng.permutation(64)[:n_even], 2 * rng.permutation(64)[:n_odd] + 1])
    v = rng.standard_normal(len(pos)).astype(np.float32)
    row[pos] = np.where(v == 0, np.float32(1.0), v)
    return row


def table_a(rng):
    """50 % kept, no row over capacity"""
    t = rng.standard_normal((NV, 128)).astype(np.float32)
    t[t == 0] = 1.0
    t *= rng.random((NV, 128)) < 0.5
    t[t == 0] = 0.0  # (no -0.0 from the product)
    ev, od = half_counts(t)
    for r in np.nonzero((ev > CAP) | (od > CAP))[0]:
        t[r] = row_with(rng, min(int(ev[r]), CAP), min(int(od[r]), CAP))
    return t


def over_kinds(rng):
    """the three ways over capacity: 47 values in the even half only, in the odd half only, every value kept"""
    return [row_with(rng, CAP + 1, int(rng.integers(0, CAP + 1))), row_with(rng, int(rng.integers(0, CAP + 1)), CAP + 1),
            row_with(rng, 64, 64)]


def make_tables(col):
    rng = np.random.default_rng(202)
    a = table_a(rng)
    tabs = {"A": a}
    rb = int(np.bincount(col, minlength=NV).argmax())  # the table row most rows gather
    for name, row in zip(("B_even", "B_odd", "B_dense"), over_kinds(rng)):
        t = a.copy()
        t[rb] = row
        tabs[name] = t
    c = a.copy()
    for i, r in enumerate(range(3, NV, 8)):
        c[r] = over_kinds(rng)[i % 3]
    tabs["C"] = c
    d = a.copy()
    for r in range(NV):
        d[r] = over_kinds(rng)[r % 3]
    tabs["D"] = d
    e = a.copy()
    for r in range(NV):
        e[r] = row_with(rng, CAP, CAP) if r % 2 == 0 else row_with(rng, CAP + 1, 0)
    tabs["E"] = e
    return tabs


def over_rows_of(t):
    ev, od = half_counts(t)
    return (ev > CAP) | (od > CAP)


@pytest.fixture(scope="module")
def case(ctx):
    rowptr, col = build_graph()
    tabs = make_tables(col)
    # conditions on the inputs, before the GPU is used
    deg = np.diff(rowptr)
    assert set(DEGREES) <= set(deg.tolist()) and sorted(deg[deg > HEAVY].tolist()) == [1025, 1300]
    over = {k: over_rows_of(t) for k, t in tabs.items()}
    assert over["A"].sum() == 0
    for k in ("B_even", "B_odd", "B_dense"):
        assert over[k].sum() == 1, k
    ev, od = half_counts(tabs["B_even"][over["B_even"]])
    assert ev[0] == CAP + 1 and od[0] <= CAP
    ev, od = half_counts(tabs["B_odd"][over["B_odd"]])
    assert od[0] == CAP + 1 and ev[0] <= CAP
    assert over["C"].sum() == len(range(3, NV, 8)) and over["D"].all()
    ev, od = half_counts(tabs["E"])
    assert (ev[0::2] == CAP).all() and (od[0::2] == CAP).all() and not over["E"][0::2].any()
    assert (ev[1::2] == CAP + 1).all() and (od[1::2] == 0).all() and over["E"][1::2].all()
    full, tail = set(), set()
    for k in ("B_even", "C"):  # (the three B tables put the same row over capacity)
        f, t = slots_hit(rowptr, col, over[k])
        full |= f
        tail |= t
    assert full == set(range(U)), sorted(set(range(U)) - full)
    assert tail == TAIL_SLOTS, sorted(TAIL_SLOTS - tail)
    fb, tb = slots_hit(rowptr, col, over["B_even"])
    assert fb and tb  # the single row alone is met in batches and in tails
    g = ctx.graph(rowptr, col)
    assert ctx.graph_stats(g)["n_heavy"] == 2
    ctx.set_option("spmm_flat", 0)  # (the row form, whatever the mean degree says)
    try:
        yield g, tabs
    finally:
        ctx.set_option("spmm_flat", -1)
        g.close()


FLAGS = [dict(agg_scratch=True), dict(relu=True), dict(accumulate=True)]  # the headline call, and once each relu and accumulate


@pytest.mark.parametrize("name", ["A", "B_even", "B_odd", "B_dense", "C", "D", "E"])
def test_groups_bit_identical(ctx, case, name):
    g, tabs = case
    x = torch.from_numpy(tabs[name]).cuda()
    zs = ctx.pack_zs(x)
    gen = torch.Generator(device="cuda").manual_seed(7)
    W = torch.randn(128, 128, device="cuda", generator=gen) * 0.2
    agg0 = torch.randn(NV, 128, device="cuda", generator=gen)
    out0 = torch.randn(NV, 128, device="cuda", generator=gen)
    for kind in (capi.W_GCN, capi.W_MEAN):
        for flags in FLAGS:
            agg_r, agg_z, out_r, out_z = agg0.clone(), agg0.clone(), out0.clone(), out0.clone()
            ctx.spmm_gemm(g, kind, x, agg_r, W, out_r, transW=True, **flags)
            assert ctx.spmm_gemm_zs(g, kind, x, zs, agg_z, W, out_z, transW=True, **flags), "refused"
            what = (name, kind, flags)
            assert torch.equal(bits32(out_z), bits32(out_r)), ("out", what)
            if flags.get("agg_scratch"):
                assert torch.equal(bits32(agg_z), bits32(agg0)), ("scratch agg touched", what)
            else:
                assert torch.equal(bits32(agg_z), bits32(agg_r)), ("agg", what)
