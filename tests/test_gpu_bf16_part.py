"""GPU suite, bf16 feature tables on vertex-range partitions (csrc/spmm_part_bf16.hip, gaib_spmm_part_bf16,
gaib_spmm_gemm_part_bf16, gaib_halo_exchange_*_bf16, LearningGraph with agg_bf16 on a halo plan / set_halo_bf16, the trainer
with GAIB_RANKS > 1):

  1-5  the class kernels over bf16 tables bit for bit against the fp32 class kernels on the tables widened to fp32 -- plain and
       fused, every class graph, the 64-bit address path, the edge cases, the halo-column half piece by piece;
  6    the exchange carrying bf16 rows between processes (ipc and the strict RCCL double): the peers' bits, half the bytes, the
       odd-length and wrong-type refusals;
  7    GCN / SAGE layers on 2 and 3 ranks in the three partition modes: the bits of the fp32 partitioned layer on
       bf16-representable input, the rounding bound of tests/test_gpu_bf16.py against the oracle's GLOBAL run otherwise;
  8    a driver's own exchange through set_halo_bf16;
  9    the trainer on two ranks.
"""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from graphaibench_amd import capi
from test_gpu_classes import KINDS, Shard, dev, feat, make_shard

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED = -1, -5


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def noise(n, d, seed):
    """non-zero previous contents of an output: rows outside a class's row map must keep them, accumulate mode continues them"""
    return torch.randn(n, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


_SHARDS = {}


def shard(ctx, selfloop=True, seed=5, lo=900, hi=2100, hub=1500):
    """make_shard, built once per argument set and shared (read-only) by the tests below"""
    key = (selfloop, seed, lo, hi, hub)
    if key not in _SHARDS:
        _SHARDS[key] = make_shard(ctx, selfloop=selfloop, seed=seed, lo=lo, hi=hi, hub=hub)
    return _SHARDS[key]


def tables(ctx, g_o, s, d, seed):
    """(owned, halo) as bf16 tables and the same tables widened to fp32"""
    xo, xh = s.tables(feat(g_o.nv, d, seed))
    xo_b, xh_b = ctx.cast_f32_bf16(xo), ctx.cast_f32_bf16(xh)
    return xo_b, xh_b, ctx.cast_bf16_f32(xo_b), ctx.cast_bf16_f32(xh_b)


# ---- 1. plain class kernels ---------------------------------------------------------------------------------------------
# (300 and 520 next to the issue's widths: two column tiles of 8-byte gathers, and the 16-byte gather of rows above 512 columns)
@pytest.mark.parametrize("d", [16, 47, 64, 128, 200, 256, 300, 520])
@pytest.mark.parametrize("kind,name", KINDS)
def test_plain_class_kernels_bit_identical(ctx, d, kind, name):
    g_o, s = shard(ctx, selfloop=(kind == capi.W_GCN))
    xo_b, xh_b, xo_w, xh_w = tables(ctx, g_o, s, d, 11)
    c = s.cls
    assert c["interior"].ne > 0 and c["bnd_own"].ne > 0 and c["bnd_halo"].ne > 0 and c["bnd_full"].ne > 0
    for relu in (False, True):
        for cname, acc in (("interior", False), ("bnd_own", False), ("bnd_halo", True)):
            t32, t16 = (xh_w, xh_b) if cname == "bnd_halo" else (xo_w, xo_b)
            ref, got = noise(s.n, d, 3), noise(s.n, d, 3)
            ctx.spmm(c[cname], kind, t32, ref, accumulate=acc, relu=relu)
            ctx.spmm_part_bf16(c[cname], kind, t16, None, 0, got, accumulate=acc, relu=relu)
            assert same(got, ref), (cname, relu)
            rows = c[cname].row_map().cpu().numpy().astype(np.int64)
            outside = np.setdiff1d(np.arange(s.n), rows)
            assert len(outside) > 0 and torch.equal(got.cpu()[outside], noise(s.n, d, 3).cpu()[outside]), cname
        ref, got = noise(s.n, d, 4), noise(s.n, d, 4)
        ctx.spmm_2t(c["bnd_full"], kind, xo_w, xh_w, s.n, ref, relu=relu)
        ctx.spmm_part_bf16(c["bnd_full"], kind, xo_b, xh_b, s.n, got, relu=relu)
        assert same(got, ref), ("bnd_full", relu)
    # graphs without a row map: the round-3 split (owned-column graph, rectangular halo-column graph in accumulate mode)
    ref, got = noise(s.n, d, 5), noise(s.n, d, 5)
    ctx.spmm(s.g_own, kind, xo_w, ref)
    ctx.spmm(s.g_halo, kind, xh_w, ref, accumulate=True, relu=True)
    ctx.spmm_part_bf16(s.g_own, kind, xo_b, None, 0, got)
    ctx.spmm_part_bf16(s.g_halo, kind, xh_b, None, 0, got, accumulate=True, relu=True)
    assert same(got, ref)


# ---- 2. fused class kernels ---------------------------------------------------------------------------------------------
def fused_pair(ctx, g, kind, t32, t16, x2_32, x2_16, n_first, n, din, dout, W, seed, **kw):
    """(agg, y) of the fp32 call and of the bf16 call from the same previous contents"""
    res = []
    for bf in (False, True):
        agg, y = noise(n, din, seed), noise(n, dout, seed + 1)
        if bf:
            ctx.spmm_gemm_part_bf16(g, kind, t16, x2_16, n_first, agg, W, y, **kw)
        elif x2_32 is not None:
            ctx.spmm_gemm_2t(g, kind, t32, x2_32, n_first, agg, W, y, **kw)
        else:
            ctx.spmm_gemm(g, kind, t32, agg, W, y, **kw)
        res.append((agg, y))
    return res


@pytest.mark.parametrize("din,dout", [(128, 128), (64, 64), (64, 32)])
@pytest.mark.parametrize("kind,name", KINDS)
@pytest.mark.parametrize("transW", [False, True])
def test_fused_class_kernels_bit_identical(ctx, din, dout, kind, name, transW):
    g_o, s = shard(ctx, selfloop=(kind == capi.W_GCN), seed=8)
    assert ctx.spmm_gemm_fusable(kind, din, dout)
    xo_b, xh_b, xo_w, xh_w = tables(ctx, g_o, s, din, 3)
    W = dev(feat(dout, din, 4) if transW else feat(din, dout, 4))
    c = s.cls
    kw = dict(transW=transW, relu=True)
    (a32, y32), (a16, y16) = fused_pair(ctx, c["interior"], kind, xo_w, xo_b, None, None, 0, s.n, din, dout, W, 20, **kw)
    assert same(a16, a32) and same(y16, y32)
    # the column split of the boundary rows: owned columns plain, the halo-column half continues the sums and carries the product
    ctx.spmm(c["bnd_own"], kind, xo_w, a32)
    ctx.spmm_part_bf16(c["bnd_own"], kind, xo_b, None, 0, a16)
    assert same(a16, a32)
    ctx.spmm_gemm(c["bnd_halo"], kind, xh_w, a32, W, y32, accumulate=True, **kw)
    ctx.spmm_gemm_part_bf16(c["bnd_halo"], kind, xh_b, None, 0, a16, W, y16, accumulate=True, **kw)
    assert same(a16, a32) and same(y16, y32)
    assert np.isfinite(y16.cpu().numpy()).all()
    # one pass over [owned | halo]
    (a32, y32), (a16, y16) = fused_pair(ctx, c["bnd_full"], kind, xo_w, xo_b, xh_w, xh_b, s.n, s.n, din, dout, W, 30, **kw)
    assert same(a16, a32) and same(y16, y32)
    # the aggregate as scratch, and GAIB_OVERLAPS_TRANSFER set (no communicator here: the flag must change nothing)
    (_, y32s), (_, y16s) = fused_pair(ctx, c["bnd_full"], kind, xo_w, xo_b, xh_w, xh_b, s.n, s.n, din, dout, W, 30,
                                      agg_scratch=True, **kw)
    assert same(y16s, y32s) and same(y16s, y16)
    a_o, y_o = noise(s.n, din, 30), noise(s.n, dout, 31)
    ctx.spmm_gemm_part_bf16(c["bnd_full"], kind, xo_b, xh_b, s.n, a_o, W, y_o, overlaps_transfer=True, **kw)
    assert same(a_o, a16) and same(y_o, y16)
    a_o, y_o = noise(s.n, din, 20), noise(s.n, dout, 21)
    ctx.spmm_gemm_part_bf16(c["interior"], kind, xo_b, None, 0, a_o, W, y_o, overlaps_transfer=True, **kw)
    ref_a, ref_y = noise(s.n, din, 20), noise(s.n, dout, 21)
    ctx.spmm_gemm(c["interior"], kind, xo_w, ref_a, W, ref_y, **kw)
    assert same(a_o, ref_a) and same(y_o, ref_y)


@pytest.mark.parametrize("din,dout", [(128, 128), (64, 64)])
def test_fused_two_products_bit_identical(ctx, din, dout):
    """SAGE's self term in the same store: rows2 (fp32) through the row map"""
    g_o, s = shard(ctx, selfloop=False, seed=9)
    kind = capi.W_MEAN
    xo_b, xh_b, xo_w, xh_w = tables(ctx, g_o, s, din, 5)
    rows2 = dev(feat(s.n, din, 8))
    W, W2 = dev(feat(din, dout, 6)), dev(feat(din, dout, 7))
    c = s.cls
    kw = dict(rows2=rows2, W2=W2)
    (a32, y32), (a16, y16) = fused_pair(ctx, c["interior"], kind, xo_w, xo_b, None, None, 0, s.n, din, dout, W, 40, **kw)
    assert same(a16, a32) and same(y16, y32)
    ctx.spmm(c["bnd_own"], kind, xo_w, a32)
    ctx.spmm_part_bf16(c["bnd_own"], kind, xo_b, None, 0, a16)
    ctx.spmm_gemm(c["bnd_halo"], kind, xh_w, a32, W, y32, accumulate=True, **kw)
    ctx.spmm_gemm_part_bf16(c["bnd_halo"], kind, xh_b, None, 0, a16, W, y16, accumulate=True, **kw)
    assert same(a16, a32) and same(y16, y32)
    (a32, y32), (a16, y16) = fused_pair(ctx, c["bnd_full"], kind, xo_w, xo_b, xh_w, xh_b, s.n, s.n, din, dout, W, 50, **kw)
    assert same(a16, a32) and same(y16, y32)


@pytest.mark.parametrize("ring", [0, 1])
@pytest.mark.parametrize("kind,name", KINDS)
def test_fused_edge_stream_bit_identical(ctx, kind, name, ring):
    """the edge-stream form (spmm_flat = 1) in batches and as a software pipeline, on the continued halo-column half, the
    interior rows and the one pass over two tables"""
    g_o, s = shard(ctx, selfloop=(kind == capi.W_GCN), seed=21)
    d = 128
    xo_b, xh_b, xo_w, xh_w = tables(ctx, g_o, s, d, 3)
    W = dev(feat(d, d, 4))
    c = s.cls
    ctx.set_option("spmm_flat", 1)
    ctx.set_option("spmm_flat_ring", ring)
    try:
        (a32, y32), (a16, y16) = fused_pair(ctx, c["interior"], kind, xo_w, xo_b, None, None, 0, s.n, d, d, W, 60)
        assert same(a16, a32) and same(y16, y32)
        ctx.spmm(c["bnd_own"], kind, xo_w, a32)
        ctx.spmm_part_bf16(c["bnd_own"], kind, xo_b, None, 0, a16)
        ctx.spmm_gemm(c["bnd_halo"], kind, xh_w, a32, W, y32, accumulate=True)
        ctx.spmm_gemm_part_bf16(c["bnd_halo"], kind, xh_b, None, 0, a16, W, y16, accumulate=True)
        assert same(a16, a32) and same(y16, y32)
        (a32, y32), (a16, y16) = fused_pair(ctx, c["bnd_full"], kind, xo_w, xo_b, xh_w, xh_b, s.n, s.n, d, d, W, 70)
        assert same(a16, a32) and same(y16, y32)
    finally:
        ctx.set_option("spmm_flat", -1)
        ctx.set_option("spmm_flat_ring", -1)


@pytest.mark.parametrize("din,dout", [(100, 128), (128, 47), (200, 64)])
def test_class_graph_shapes_refused_alike(ctx, din, dout):
    """a class graph returns from the bf16 call exactly what the fp32 call returns: GAIB_ERR_UNSUPPORTED where
    gaib_spmm_gemm_fusable answers 0 -- (200, 64) does; (100, 128) and (128, 47) are padded to the kernel's tiles and fuse with
    the default options, so they are pinned to the refusal with "spmm_fuse" = 0 as well -- and nothing is written on the way"""
    g_o, s = shard(ctx, seed=8)
    kind = capi.W_GCN
    xo_b, xh_b, xo_w, xh_w = tables(ctx, g_o, s, din, 3)
    W = dev(feat(din, dout, 4))
    c = s.cls

    def both():
        rcs = []
        for bf in (False, True):
            agg, y = torch.full((s.n, din), 7.0, device="cuda"), torch.full((s.n, dout), 7.0, device="cuda")
            fn = ctx.lib.gaib_spmm_gemm_part_bf16 if bf else ctx.lib.gaib_spmm_gemm_2t
            rc = fn(ctx.h, c["bnd_full"].h, kind, None, din, (xo_b if bf else xo_w).data_ptr(), (xh_b if bf else xh_w).data_ptr(),
                    s.n, agg.data_ptr(), W.data_ptr(), 0, None, None, dout, y.data_ptr(), 0)
            ctx.sync()
            rcs.append((rc, agg, y))
        return rcs

    (rc32, a32, y32), (rc16, a16, y16) = both()
    assert rc32 == rc16, (rc32, rc16)
    if not ctx.spmm_gemm_fusable(kind, din, dout):
        assert rc16 == ERR_UNSUPPORTED and bool((y16 == 7.0).all()) and bool((a16 == 7.0).all())
    else:
        assert rc16 == 0 and same(a16, a32) and same(y16, y32)
    ctx.set_option("spmm_fuse", 0)
    try:
        assert not ctx.spmm_gemm_fusable(kind, din, dout)
        (rc32, _, _), (rc16, a16, y16) = both()
    finally:
        ctx.set_option("spmm_fuse", 1)
    assert rc32 == rc16 == ERR_UNSUPPORTED
    assert bool((y16 == 7.0).all()) and bool((a16 == 7.0).all())


def test_existing_bf16_entry_points_keep_their_refusals(ctx):
    g_o, s = shard(ctx, seed=8)
    xo_b, _, _, _ = tables(ctx, g_o, s, 128, 3)
    W = dev(feat(128, 128, 4))
    agg, y = torch.zeros(s.n, 128, device="cuda"), torch.zeros(s.n, 128, device="cuda")
    gi = s.cls["interior"]
    assert ctx.lib.gaib_spmm_bf16(ctx.h, gi.h, capi.W_GCN, None, 128, xo_b.data_ptr(), agg.data_ptr(), 0) == ERR_UNSUPPORTED
    rc = ctx.lib.gaib_spmm_gemm_bf16(ctx.h, gi.h, capi.W_GCN, None, 128, xo_b.data_ptr(), agg.data_ptr(), W.data_ptr(), 0, 128,
                                     y.data_ptr(), 0)
    assert rc == ERR_UNSUPPORTED and b"row map" in ctx.lib.gaib_last_error()
    rc = ctx.lib.gaib_spmm_gemm_bf16(ctx.h, s.g_own.h, capi.W_GCN, None, 128, xo_b.data_ptr(), agg.data_ptr(), W.data_ptr(), 0,
                                     128, y.data_ptr(), 8)
    assert rc == ERR_INVALID


# ---- 3. 64-bit address path ---------------------------------------------------------------------------------------------
def test_two_bf16_tables_through_64_bit_addresses(ctx):
    g_o, s = shard(ctx, seed=12)
    d = 128
    c = s.cls
    ctx.set_option("spmm_addr_mode", 2)
    try:
        for kind, _ in KINDS[:2]:
            xo_b, xh_b, xo_w, xh_w = tables(ctx, g_o, s, d, 2)
            W = dev(feat(d, d, 4))
            for relu in (False, True):
                ref, got = noise(s.n, d, 4), noise(s.n, d, 4)
                ctx.spmm_2t(c["bnd_full"], kind, xo_w, xh_w, s.n, ref, relu=relu)
                ctx.spmm_part_bf16(c["bnd_full"], kind, xo_b, xh_b, s.n, got, relu=relu)
                assert same(got, ref)
            for transW in (False, True):
                (a32, y32), (a16, y16) = fused_pair(ctx, c["bnd_full"], kind, xo_w, xo_b, xh_w, xh_b, s.n, s.n, d, d, W, 80,
                                                    transW=transW, relu=True)
                assert same(a16, a32) and same(y16, y32)
    finally:
        ctx.set_option("spmm_addr_mode", 0)
    # ... and the default mode gives the same bits (buffer descriptors)
    ref = noise(s.n, d, 4)
    ctx.spmm_part_bf16(c["bnd_full"], kind, xo_b, xh_b, s.n, ref, relu=True)
    assert same(got, ref)


# ---- 4. edge cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 3000), (0, 1), (1500, 1501)])
def test_edge_cases_bit_identical(ctx, lo, hi):
    """the whole graph (no boundary row), the hub row alone (a heavy boundary row), one ordinary row; only class graphs with at
    least one edge are aggregated (host/aggregators.cpp never launches an empty bnd_halo)"""
    g_o, s = shard(ctx, lo=lo, hi=hi, hub=2500)
    kind, d = capi.W_GCN, 128
    xo_b, xh_b, xo_w, xh_w = tables(ctx, g_o, s, d, 2)
    W = dev(feat(d, d, 4))
    c = s.cls
    n_checked = 0
    for cname in ("interior", "bnd_own", "bnd_halo", "bnd_full"):
        g = c[cname]
        if g.ne == 0:
            continue
        two = cname == "bnd_full"
        t32, t16 = (xh_w, xh_b) if cname == "bnd_halo" else (xo_w, xo_b)
        acc = cname == "bnd_halo"
        ref, got = noise(s.n, d, 6), noise(s.n, d, 6)
        if two:
            ctx.spmm_2t(g, kind, xo_w, xh_w, s.n, ref)
        else:
            ctx.spmm(g, kind, t32, ref, accumulate=acc)
        ctx.spmm_part_bf16(g, kind, t16, xh_b if two else None, s.n if two else 0, got, accumulate=acc)
        assert same(got, ref), cname
        (a32, y32), (a16, y16) = fused_pair(ctx, g, kind, t32, t16, xh_w if two else None, xh_b if two else None,
                                            s.n if two else 0, s.n, d, d, W, 90, accumulate=acc)
        assert same(a16, a32) and same(y16, y32), cname
        n_checked += 1
    assert n_checked >= (1 if hi - lo == 3000 else 2)
    if lo == 0 and hi == 1:  # the hub row: above the heavy threshold in one of the classes
        assert max(int(np.diff(s.rp_own)[0]), int(np.diff(s.rp_halo)[0])) > 1024


# ---- 5. pieces ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("peers,K", [(1, 4), (3, 2)])
def test_halo_half_piece_by_piece_bit_identical(ctx, peers, K):
    g_o, s = shard(ctx)
    kind, d = capi.W_GCN, 128
    xo_b, xh_b, xo_w, xh_w = tables(ctx, g_o, s, d, 11)
    W = dev(feat(d, d, 4))
    nh = len(s.halo)
    seg = [nh * p // peers for p in range(peers + 1)]
    ranges = []
    for p in range(peers):
        r = seg[p + 1] - seg[p]
        ranges += [(seg[p] + r * k // K, seg[p] + r * (k + 1) // K, k) for k in range(K)]
    pieces = ctx.split_pieces(s.cls["bnd_halo"], K, ranges)
    assert sum(p.ne for p in pieces) == s.cls["bnd_halo"].ne and sum(p.ne > 0 for p in pieces) == K
    a32, a16 = noise(s.n, d, 7), noise(s.n, d, 7)
    y32, y16 = noise(s.n, d, 8), noise(s.n, d, 8)
    for k, p in enumerate(pieces):
        if k < K - 1:
            ctx.spmm(p, kind, xh_w, a32, accumulate=True)
            ctx.spmm_part_bf16(p, kind, xh_b, None, 0, a16, accumulate=True)
        else:  # the last piece carries the product
            ctx.spmm_gemm(p, kind, xh_w, a32, W, y32, accumulate=True, relu=True)
            ctx.spmm_gemm_part_bf16(p, kind, xh_b, None, 0, a16, W, y16, accumulate=True, relu=True)
        assert same(a16, a32), k
    assert same(y16, y32)
    for p in pieces:
        p.close()


# ---- 6. the exchange ------------------------------------------------------------------------------------------------------
def _exchange_worker(rank, world, idfile, q, transport_name, chunk_bytes):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["GAIB_COMM_TIMEOUT_S"] = "60"
    if chunk_bytes:
        os.environ["GAIB_IPC_CHUNK_BYTES"] = str(chunk_bytes)
    try:
        from graphaibench_amd import capi, layers as L
        from test_gpu_comm import _id_via_file, _transport

        ctx = L.init(0)
        transport = _transport(transport_name, capi)
        comm = capi.Comm(ctx, rank, world, _id_via_file(idfile, rank, transport, capi), transport)
        n_own = 3000
        rng = np.random.default_rng(100)  # the same plan on every rank: rank r needs rows need[r][q] of rank q
        need = [[np.sort(rng.choice(n_own, 500 + 50 * (r + q), replace=False)) if q != r else np.empty(0, np.int64)
                 for q in range(world)] for r in range(world)]
        send_idx = np.concatenate([need[q][rank] for q in range(world)]).astype(np.int64)
        send_counts = [len(need[q][rank]) for q in range(world)]
        recv_counts = [len(need[rank][q]) for q in range(world)]

        def rows_of(r, length, salt):  # rank r's rows as bf16 bits (int16), reproducible on every rank
            x = torch.from_numpy(np.random.default_rng(1000 * r + length + salt).standard_normal((n_own, length)).astype(np.float32))
            return x.to(torch.bfloat16).view(torch.int16).numpy()

        halo = comm.halo(send_counts, send_idx, recv_counts)
        salt = 0
        for K in (1, 2):
            halo.set_pieces(K)
            for length in (128, 6):
                salt += 1
                mine = torch.from_numpy(rows_of(rank, length, salt)).cuda().view(torch.bfloat16)
                b0 = halo.bytes_sent
                halo.begin_bf16(mine, length)
                if K > 1:
                    for k in range(K):
                        halo.wait_piece_bf16(k)
                ptr = halo.end_bf16()
                ctx.sync()
                sent16 = halo.bytes_sent - b0
                got = torch.empty(max(halo.rows, 1), length, dtype=torch.int16, device="cuda")
                capi._check(ctx.lib.gaib_memcpy_d2d(ctx.h, got.data_ptr(), ptr, halo.rows * length * 2), "d2d")
                ctx.sync()
                want = np.concatenate([rows_of(q, length, salt)[need[rank][q]] for q in range(world)])
                assert np.array_equal(got[:halo.rows].cpu().numpy(), want), f"bf16 exchange len {length} K {K}"
                # the fp32 exchange of the same plan and len moves exactly twice the bytes
                f32 = torch.zeros(n_own, length, device="cuda")
                b0 = halo.bytes_sent
                halo.begin(f32, length)
                halo.end()
                ctx.sync()
                assert sent16 > 0 and 2 * sent16 == halo.bytes_sent - b0, (sent16, halo.bytes_sent - b0)
        if chunk_bytes:
            assert 128 * 2 * len(send_idx) > chunk_bytes  # (the send buffer of the long rows did travel in chunks)
        # an odd length is refused locally on every rank, nothing is left pending: an even exchange follows on the same plan
        odd = torch.zeros(n_own, 7, dtype=torch.bfloat16, device="cuda")
        assert ctx.lib.gaib_halo_exchange_begin_bf16(halo.h, 7, odd.data_ptr()) == ERR_UNSUPPORTED
        mine = torch.from_numpy(rows_of(rank, 8, 99)).cuda().view(torch.bfloat16)
        halo.begin_bf16(mine, 8)
        # ... which the other element type's functions refuse to end or to wait for; the exchange stays in flight
        import ctypes as C
        p = C.c_void_p()
        assert ctx.lib.gaib_halo_exchange_end(halo.h, C.byref(p)) == ERR_INVALID
        assert ctx.lib.gaib_halo_exchange_wait_piece(halo.h, 0, C.byref(p)) == ERR_INVALID
        ptr = halo.end_bf16()
        ctx.sync()
        got = torch.empty(max(halo.rows, 1), 8, dtype=torch.int16, device="cuda")
        capi._check(ctx.lib.gaib_memcpy_d2d(ctx.h, got.data_ptr(), ptr, halo.rows * 8 * 2), "d2d")
        ctx.sync()
        assert np.array_equal(got[:halo.rows].cpu().numpy(), np.concatenate([rows_of(q, 8, 99)[need[rank][q]] for q in range(world)]))
        halo.begin(torch.zeros(n_own, 8, device="cuda"), 8)
        assert ctx.lib.gaib_halo_exchange_end_bf16(halo.h, C.byref(p)) == ERR_INVALID
        assert ctx.lib.gaib_halo_exchange_wait_piece_bf16(halo.h, 0, C.byref(p)) == ERR_INVALID
        halo.end()
        comm.barrier()
        halo.close()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, "FAIL: " + traceback.format_exc()))


@pytest.mark.parametrize("transport_name,world,chunk_bytes", [("ipc", 2, 0), ("ipc", 3, 50000), ("fake-rccl", 2, 0),
                                                             ("fake-rccl", 3, 0)])
def test_exchange_carries_bf16_rows(tmp_path, transport_name, world, chunk_bytes):
    from test_gpu_comm import _spawn

    res = _spawn(world, _exchange_worker, (str(tmp_path / "id"), transport_name, chunk_bytes), timeout=120)
    assert all(r[1] == "ok" for r in res), res


# ---- 7. layers on a partition ---------------------------------------------------------------------------------------------
def _bf16_exact(a):
    """the fp32 array rounded to bf16-representable values"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()


def _layer_worker(rank, world, idfile, q, arch, mode, din, dout, K, transport_name, odd_too):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["GAIB_COMM_TIMEOUT_S"] = "60"
    os.environ["GAIB_PART_MODE"] = mode
    if K > 1:
        os.environ["GAIB_HALO_PIECES"] = str(K)
        os.environ["GAIB_HALO_CONSUME"] = str(K)
    try:
        from graphaibench_amd import capi, layers as L
        from oracle import binding as orc
        from test_gpu_bf16 import dense_ops, within
        from test_gpu_comm import _id_via_file, _transport
        from util import LONG_SUM_FLOOR, assert_close, random_graph

        transport = _transport(transport_name, capi)
        ctx = L.init(0)
        comm = capi.Comm(ctx, rank, world, _id_via_file(idfile, rank, transport, capi), transport)
        L.set_comm(comm)
        gcn = arch == "gcn"
        rp, ci = random_graph(3000, 10, seed=17, power_law=True, hub_deg=1500)
        g = orc.Graph(rp, ci)
        if gcn:
            g = g.add_selfloop()
        n = g.nv
        x = np.random.default_rng(5).standard_normal((n, din)).astype(np.float32)
        gin = np.random.default_rng(6).standard_normal((n, dout)).astype(np.float32)
        part = L.HostPartition(g.rowptr, g.colidx, rank, world)
        lo, hi = part.lo, part.hi
        lg = part.make_graph(comm)
        used, n_bnd, _ = lg.partition_mode(din)
        assert L.LGraph.PART_NAMES[used] == mode, (used, mode)
        if K > 1:
            assert lg.halo_pieces(din) == K
        kind = L.GCN if gcn else L.SAGE

        def run(xg, bf16, d_in=din, d_out=dout, g_in=gin):
            ctx.set_option("agg_bf16", 1 if bf16 else 0)
            layer = L.Layer(kind, 1, hi - lo, d_in, d_out, lg, False)
            layer.write(L.FEAT_IN, torch.from_numpy(xg[lo:hi]).cuda())
            out = torch.full((hi - lo, d_out), float("nan"), device="cuda")
            layer.forward(out)
            layer.write(L.GRAD_IN, torch.from_numpy(g_in[lo:hi]).cuda())
            go = torch.full((hi - lo, d_in), float("nan"), device="cuda")
            layer.backward(out, go)
            L.sync()
            r = dict(out=out.cpu().numpy(), go=go.cpu().numpy(), W=layer.tensor(L.W_NEIGH, (d_in, d_out)).cpu().numpy().astype(np.float64))
            if not gcn:
                r["Ws"] = layer.tensor(L.W_SELF, (d_in, d_out)).cpu().numpy().astype(np.float64)
            layer.update_weight(L.adam(0.01))  # (sums the gradients over the ranks first)
            r["Wg"] = layer.tensor(L.W_NEIGH_GRAD, (d_in, d_out)).cpu().numpy()
            if not gcn:
                r["Wsg"] = layer.tensor(L.W_SELF_GRAD, (d_in, d_out)).cpu().numpy()
            comm.barrier()
            layer.close()
            ctx.set_option("agg_bf16", 0)
            return r

        # (a) bf16-representable features: the bits of the fp32 partitioned layer's forward
        xr = _bf16_exact(x)
        r32, r16 = run(xr, False), run(xr, True)
        assert np.isfinite(r16["out"]).all() and np.isfinite(r16["go"]).all()
        assert np.array_equal(r16["out"].view(np.uint32), r32["out"].view(np.uint32)), "forward on representable features"
        # (b) against the oracle's GLOBAL run, within one bf16 rounding of the gathered table (tests/test_gpu_bf16.py's bound)
        lo_ = (orc.GCNLayer if gcn else orc.SAGELayer)(1, g, din, dout, False)
        want, want_go = lo_.forward(x), lo_.backward(gin.copy())
        r = run(x, True)
        A, At = dense_ops(np.asarray(g.rowptr, np.int64), np.asarray(g.colidx, np.uint32), n, gcn)
        aX, aG, aW = np.abs(x.astype(np.float64)), np.abs(gin.astype(np.float64)), np.abs(r["W"])
        aWs = np.abs(r["Ws"]) if not gcn else None
        bound = (A @ aX @ aW)[lo:hi]
        within(r["out"], want[lo:hi].astype(np.float64), bound, bound + ((aX @ aWs)[lo:hi] if not gcn else 0), f"{arch} forward")
        bound_wg = aX.T @ At @ aG
        within(r["Wg"], (lo_.W_grad if gcn else lo_.W_neigh_grad).astype(np.float64), bound_wg, bound_wg, f"{arch} W_neigh_grad")
        if not gcn:
            within(r["Wsg"], lo_.W_self_grad.astype(np.float64), 0.0, aX.T @ aG, "sage W_self_grad")
        bound_go = (At @ aG @ aW.T)[lo:hi]
        within(r["go"], want_go[lo:hi].astype(np.float64), bound_go, bound_go + ((aG @ aWs.T)[lo:hi] if not gcn else 0),
               f"{arch} grad_out")
        # (c) and the rounding shows: on features that are not representable the bf16 path is not the fp32 one
        r32x = run(x, False)
        assert not np.array_equal(r["out"].view(np.uint32), r32x["out"].view(np.uint32))
        assert not np.array_equal(r["go"].view(np.uint32), r32x["go"].view(np.uint32))
        if odd_too:
            # (d) 128 -> 47: the layer multiplies first and aggregates 47 columns -- an odd width runs on the fp32 path, with
            # agg_bf16 on, and meets the fp32 tolerance
            gin47 = np.random.default_rng(7).standard_normal((n, 47)).astype(np.float32)
            x128 = np.random.default_rng(8).standard_normal((n, 128)).astype(np.float32)
            l47 = (orc.GCNLayer if gcn else orc.SAGELayer)(1, g, 128, 47, False)
            w47, wgo47 = l47.forward(x128), l47.backward(gin47.copy())
            r47 = run(x128, True, 128, 47, gin47)
            assert_close(r47["out"], w47[lo:hi], "128 -> 47 forward", floor=LONG_SUM_FLOOR)
            assert_close(r47["go"], wgo47[lo:hi], "128 -> 47 grad_out", floor=LONG_SUM_FLOOR)
            assert_close(r47["Wg"], l47.W_grad if gcn else l47.W_neigh_grad, "128 -> 47 W_grad", floor=LONG_SUM_FLOOR)
        comm.barrier()
        lg.close()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, "FAIL: " + traceback.format_exc()))


@pytest.mark.parametrize("arch,world,mode,din,dout,K,transport_name,odd_too", [
    ("gcn", 2, "split", 128, 128, 1, "ipc", True), ("gcn", 2, "classes", 128, 128, 1, "ipc", False),
    ("gcn", 2, "onepass", 128, 128, 1, "ipc", False), ("sage", 3, "split", 128, 128, 1, "ipc", False),
    ("sage", 3, "classes", 128, 128, 1, "ipc", False), ("sage", 3, "onepass", 128, 128, 1, "ipc", True),
    ("gcn", 3, "split", 64, 64, 1, "ipc", False), ("gcn", 2, "classes", 128, 128, 2, "fake-rccl", False)])
def test_layers_with_bf16_tables_on_a_partition(tmp_path, arch, world, mode, din, dout, K, transport_name, odd_too):
    from test_gpu_comm import _spawn

    res = _spawn(world, _layer_worker, (str(tmp_path / "id"), arch, mode, din, dout, K, transport_name, odd_too), timeout=240)
    assert all(r[1] == "ok" for r in res), res


# ---- 8. a driver's own exchange: set_halo_bf16 -------------------------------------------------------------------------------
def test_layer_over_bf16_callbacks():
    """one rank of a simulated partition: the callbacks receive the owned rows as bf16 bits and hand back a pre-filled bf16 halo
    table (the features' halo rows in forward, the gradient's in backward); a GCN layer against the oracle on the GLOBAL graph"""
    from graphaibench_amd import layers as L
    from oracle import binding as orc
    from test_gpu_bf16 import dense_ops, within

    lctx = L.init(0)
    g_o, s = make_shard(lctx)
    n, d, lo, hi = g_o.nv, 128, s.lo, s.hi
    x, gin = feat(n, d, 21), feat(n, d, 22)
    halo_x = lctx.cast_f32_bf16(dev(x[s.halo]))
    halo_g = lctx.cast_f32_bf16(dev(gin[s.halo]))
    seen = []

    def begin(length, ptr):
        assert length == d and ptr
        got = torch.empty(s.n, d, dtype=torch.int16, device="cuda")
        capi._check(lctx.lib.gaib_memcpy_d2d(lctx.h, got.data_ptr(), ptr, s.n * d * 2), "d2d")
        lctx.sync()
        seen.append(got.cpu())

    def end(length):
        return (halo_x if len(seen) == 1 else halo_g).data_ptr()

    lg = L.LGraph.adopt(s.g_own)
    lg.set_halo_bf16(s.g_halo, begin, end)
    lctx.set_option("agg_bf16", 1)
    try:
        layer = L.Layer(L.GCN, 1, s.n, d, d, lg, False)
        layer.write(L.FEAT_IN, dev(x[lo:hi]))
        out = torch.full((s.n, d), float("nan"), device="cuda")
        layer.forward(out)
        layer.write(L.GRAD_IN, dev(gin[lo:hi]))
        go = torch.full((s.n, d), float("nan"), device="cuda")
        layer.backward(out, go)
        L.sync()
        W = layer.tensor(L.W_NEIGH, (d, d)).cpu().numpy().astype(np.float64)
        Wg = layer.tensor(L.W_NEIGH_GRAD, (d, d)).cpu().numpy()
        layer.close()
    finally:
        lctx.set_option("agg_bf16", 0)
    # the callbacks saw this rank's rows, rounded to bf16
    assert len(seen) == 2
    assert torch.equal(seen[0], torch.from_numpy(x[lo:hi]).to(torch.bfloat16).view(torch.int16))
    assert torch.equal(seen[1], torch.from_numpy(gin[lo:hi]).to(torch.bfloat16).view(torch.int16))
    lo_ = orc.GCNLayer(1, g_o, d, d, False)
    want, want_go = lo_.forward(x), lo_.backward(gin.copy())
    A, At = dense_ops(np.asarray(g_o.rowptr, np.int64), np.asarray(g_o.colidx, np.uint32), n, True)
    aX, aG, aW = np.abs(x.astype(np.float64)), np.abs(gin.astype(np.float64)), np.abs(W)
    bound = (A @ aX @ aW)[lo:hi]
    within(out.cpu().numpy(), want[lo:hi].astype(np.float64), bound, bound, "forward")
    bound_go = (At @ aG @ aW.T)[lo:hi]
    within(go.cpu().numpy(), want_go[lo:hi].astype(np.float64), bound_go, bound_go, "grad_out")
    # this rank's share of the weight gradient: (A X)[rows]^T G[rows]
    AX = A @ x.astype(np.float64)
    bound_wg = (A @ aX)[lo:hi].T @ aG[lo:hi]
    within(Wg, AX[lo:hi].T @ gin[lo:hi].astype(np.float64), bound_wg, bound_wg, "W_grad share")
    lg.close()


def test_bf16_callbacks_take_the_exchange_whole_where_the_fp32_pair_has_pieces():
    """a driver whose fp32 callbacks land in slices (set_halo_pieces) and that also gives bf16 callbacks: under agg_bf16 an
    even-width aggregation consumes the bf16 table in ONE piece (the bf16 pair has no wait_piece), an odd width keeps the pieces"""
    from graphaibench_amd import layers as L

    lctx = L.init(0)
    g_o, s = make_shard(lctx, seed=6)
    d = 128
    x = feat(g_o.nv, d, 23)
    halo_x = lctx.cast_f32_bf16(dev(x[s.halo]))
    nh = len(s.halo)
    lg = L.LGraph.adopt(s.g_own)
    lg.set_halo(s.g_halo, lambda n, p: None, lambda n: 0)
    lg.set_halo_bf16(s.g_halo, lambda n, p: None, lambda n: halo_x.data_ptr())
    lg.set_halo_pieces(2, [(0, nh // 2, 0), (nh // 2, nh, 1)], lambda k: 0)
    lg.set_halo_consumption(2)
    lg.set_partition_mode(L.LGraph.PART_SPLIT)
    assert L.LGraph.PART_NAMES[lg.partition_mode(d)[0]] == "split"
    assert lg.halo_pieces(d) == 2
    lctx.set_option("agg_bf16", 1)
    try:
        assert lg.halo_pieces(d) == 1 and lg.halo_pieces(47) == 2
        layer = L.Layer(L.GCN, 1, s.n, d, d, lg, False)
        layer.write(L.FEAT_IN, dev(x[s.lo:s.hi]))
        out = torch.full((s.n, d), float("nan"), device="cuda")
        layer.forward(out)
        L.sync()
        assert np.isfinite(out.cpu().numpy()).all()
        layer.close()
    finally:
        lctx.set_option("agg_bf16", 0)
    lg.close()


# ---- 9. the trainer on two ranks --------------------------------------------------------------------------------------------
def test_trainer_two_ranks_with_bf16_tables(tmp_path):
    from test_gpu_bf16 import make_dataset

    root = make_dataset(tmp_path)
    exe = ROOT / "bin" / "gpu_train_gcn"
    assert exe.exists(), "run graphaibench_amd.build"
    cmd = [str(exe), "cora", "20", "2", "softmax", "64", "0", "0", "0.01", "2", "0", "4", "0"]
    finals = {}
    for ranks in ("2", "1"):
        clean = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GAIB_RANK", "GAIB_WORLD",
                                                                    "GAIB_COMM", "GAIB_DEVICE", "GAIB_COMM_ID_FILE", "GAIB_RANKS")}
        env = dict(clean, DATASET_PATH=root, GAIB_AGG_DTYPE="bf16", GAIB_EPOCH_LOSSES="1", GAIB_COMM_TIMEOUT_S="60")
        if ranks != "1":
            env["GAIB_RANKS"] = ranks
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "aggregation tables: bf16" in r.stdout
        if ranks != "1":
            assert "aggregation tables: bf16 (odd widths on a partition: fp32)" in r.stdout
        m = re.search(r"epoch_losses ([0-9eE.+\- ]+)", r.stdout + r.stderr)
        losses = [float(v) for v in m.group(1).split()] if m else [float(a) for a in re.findall(r"train_loss ([0-9.]+)", r.stdout)]
        assert len(losses) == 20, losses
        assert losses[-1] < losses[0] * 0.9, losses
        finals[ranks] = losses[-1]
    assert abs(finals["2"] - finals["1"]) <= 0.02 * finals["1"], finals
