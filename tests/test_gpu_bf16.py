"""GPU suite, bf16 feature tables: the two casts against torch's CPU conversion, gaib_spmm_bf16 bit for bit against
gaib_spmm_ex on the widened table, the GCN / SAGE layers with the context option agg_bf16 against the rounding bound, the
refusals, and the trainer with GAIB_AGG_DTYPE=bf16."""
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from graphaibench_amd import capi, layers as L
from oracle import binding as orc
from util import ELEM_FLOOR, ELEM_RTOL, random_graph

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
U_BF16 = 2.0 ** -8  # unit roundoff of bf16 (8 significant bits)


def bits32(t):
    return t.contiguous().view(torch.int32)


# ---- casts ----------------------------------------------------------------------------------------------------------
SPECIAL = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00008000, 0x00018000, 0x00017fff,
           0x3f808000, 0x3f818000, 0x3f80ffff, 0xbf808001, 0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0xff7fffff, 0x7f800000,
           0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fbfffff, 0x7fffffff, 0xffffffff, 0x7f80ffff]


def test_cast_f32_bf16_matches_torch(ctx):
    rng = np.random.default_rng(0)
    words = np.concatenate([np.array(SPECIAL, np.uint32), rng.integers(0, 2 ** 32, 1_000_000, dtype=np.uint32)])
    # every exponent, both signs, mantissas at and around the rounding point
    e = np.arange(256, dtype=np.uint32) << 23
    for low in (0x0, 0x7fff, 0x8000, 0x8001, 0x18000, 0x7fffff):
        words = np.concatenate([words, e | low, e | low | 0x80000000])
    f = words.view(np.float32)
    got = ctx.cast_f32_bf16(torch.from_numpy(f).cuda()).cpu().view(torch.int16).numpy().view(np.uint16)
    want = torch.from_numpy(f).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(f)
    assert nan.sum() > 1000
    assert np.array_equal(got[~nan], want[~nan]), np.flatnonzero(got[~nan] != want[~nan])[:10]
    # NaN: torch's CPU conversion encodes it by code path (0xffff from its vector loop, 0x7fc0 from the scalar one); the
    # contract is the class -- a quiet NaN of the same sign
    g = got[nan].astype(np.uint32)
    assert np.all((g & 0x7f80) == 0x7f80) and np.all(g & 0x0040)
    assert np.array_equal(g >> 15, words[nan] >> 31)
    # unaligned pointers: the scalar kernel, same bits
    x = torch.from_numpy(f[:100_001]).cuda()
    out = torch.empty(100_001, dtype=torch.bfloat16, device="cuda")
    ctx.cast_f32_bf16(x[1:], out[1:])
    assert np.array_equal(out[1:].cpu().view(torch.int16).numpy().view(np.uint16)[~nan[1:100_001]],
                          want[1:100_001][~nan[1:100_001]])


def test_cast_bf16_f32_is_exact(ctx):
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for off in (0, 1):  # aligned (vector kernel) and unaligned (scalar kernel)
        src = torch.from_numpy(np.concatenate([np.zeros(off, np.uint16), b]).view(np.int16)).cuda().view(torch.bfloat16)[off:]
        out = torch.empty(65536 + off, dtype=torch.float32, device="cuda")[off:]
        ctx.cast_bf16_f32(src, out)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), b.astype(np.uint32) << 16)


# ---- gaib_spmm_bf16: bit-identical to gaib_spmm_ex on the widened table -----------------------------------------------
LENS = [1, 3, 4, 8, 31, 47, 64, 100, 128, 129, 256, 513, 1024]
KINDS = [capi.W_GCN, capi.W_MEAN, capi.W_MEAN_T, capi.W_EDGE, capi.W_EDGE_T]


def csr(nrows, src, dst):
    """directed CSR over [nrows] rows (columns as given: a rectangular column space allowed), sorted, duplicate-free"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    key = np.unique(src * (dst.max() + 1 if len(dst) else 1) + dst) if len(src) else np.zeros(0, np.int64)
    m = dst.max() + 1 if len(dst) else 1
    rows, cols = key // m, (key % m).astype(np.uint32)
    rowptr = np.zeros(nrows + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr), cols


def graphs(ctx):
    n = 2000
    rp, ci = random_graph(n, 12, seed=1)
    yield "random", ctx.graph(rp, ci), n
    rp, ci = random_graph(3000, 8, seed=2, power_law=True, hub_deg=2500)  # a hub above the heavy threshold (1024)
    yield "powerlaw_hub", ctx.graph(rp, ci), 3000
    rng = np.random.default_rng(3)
    src = rng.integers(0, n, 12000)
    src = src[src % 3 != 0]  # every third row empty
    yield "empty_rows", ctx.graph(*csr(n, src, rng.integers(0, n, len(src)))), n
    yield "no_edges", ctx.graph(np.zeros(n + 1, np.int64), np.zeros(0, np.uint32)), n
    nc = 5000
    src = rng.integers(0, 1500, 20000)
    g = ctx.graph(*csr(1500, src, rng.integers(0, nc, len(src))), ncols=nc)
    pos = lambda k: torch.rand(k, device="cuda") + 0.05  # the column side's normalisers (gaib_graph_set_vertex_norm)
    g.set_vertex_norm(pos(1500), pos(nc), pos(nc), row_inv_deg=pos(1500))
    yield "rect", g, nc


def check_identity(ctx, g, nc, lens, kinds=KINDS, flag_sets=((False, False), (False, True), (True, False))):
    gen = torch.Generator(device="cuda").manual_seed(7)
    ne = g.ne
    ew = torch.rand(max(ne, 1), device="cuda", generator=gen) + 0.1
    n_checked = 0
    for ln in lens:
        xb = torch.randn(nc, ln, device="cuda", generator=gen).to(torch.bfloat16)
        xw = ctx.cast_bf16_f32(xb)
        for kind in kinds:
            w = ew if kind in (capi.W_EDGE, capi.W_EDGE_T) else None
            for acc, relu in flag_sets:
                init = torch.randn(g.nv, ln, device="cuda", generator=gen)
                ref, got = init.clone(), init.clone()
                try:
                    ctx.spmm(g, kind, xw, ref, edge_w=w, accumulate=acc, relu=relu)
                except capi.GaibError:  # (reverse-edge weights on a graph without reverse edges): refused alike
                    with pytest.raises(capi.GaibError):
                        ctx.spmm_bf16(g, kind, xb, got, edge_w=w, accumulate=acc, relu=relu)
                    continue
                ctx.spmm_bf16(g, kind, xb, got, edge_w=w, accumulate=acc, relu=relu)
                assert torch.equal(bits32(got), bits32(ref)), (ln, kind, acc, relu)
                n_checked += 1
    return n_checked


def test_spmm_bf16_bit_identical(ctx):
    total = 0
    for name, g, nc in graphs(ctx):
        lens = LENS if name in ("random", "powerlaw_hub") else [1, 47, 128, 129, 513]
        total += check_identity(ctx, g, nc, lens)
        g.close()
    assert total > 400


@pytest.mark.parametrize("layout", [4, 8])
def test_spmm_bf16_sub_wave_layouts_and_chunks(ctx, layout):
    """the A/B lane layouts (spmm_bf16_layout) and the ordered-chunk form (spmm_chunked = 1): the same bits"""
    rp, ci = random_graph(3000, 8, seed=2, power_law=True, hub_deg=2500)
    g = ctx.graph(rp, ci)
    try:
        ctx.set_option("spmm_bf16_layout", layout)
        check_identity(ctx, g, 3000, [8, 64, 100, 128, 256], kinds=[capi.W_GCN, capi.W_MEAN, capi.W_EDGE])
        ctx.set_option("spmm_bf16_layout", 0)
        ctx.set_option("spmm_chunked", 1)
        check_identity(ctx, g, 3000, [4, 64, 128, 256], kinds=[capi.W_GCN, capi.W_MEAN_T])
    finally:
        ctx.set_option("spmm_bf16_layout", 0)
        ctx.set_option("spmm_chunked", -1)
        g.close()


def test_spmm_bf16_table_above_4gb(ctx):
    """a rectangular graph whose bf16 table is 4.5 GB: the 64-bit gather path, columns at the far end of the table"""
    nv, nc, ln = 64, 2_200_000, 1024
    assert nc * ln * 2 > 2 ** 32
    rng = np.random.default_rng(5)
    src = np.repeat(np.arange(nv), 12)
    dst = np.concatenate([rng.integers(0, nc, nv * 6), rng.integers(nc - 4096, nc, nv * 6)])
    g = ctx.graph(*csr(nv, src, dst), ncols=nc)
    xb = torch.empty(nc, ln, dtype=torch.bfloat16, device="cuda")
    xb.normal_()
    xw = ctx.cast_bf16_f32(xb)
    ew = torch.rand(g.ne, device="cuda") + 0.1
    for kind, w in ((capi.W_MEAN, None), (capi.W_EDGE, ew)):
        ref, got = torch.empty(nv, ln, device="cuda"), torch.empty(nv, ln, device="cuda")
        ctx.spmm(g, kind, xw, ref, edge_w=w)
        ctx.spmm_bf16(g, kind, xb, got, edge_w=w)
        assert torch.equal(bits32(got), bits32(ref))
    del xw, xb
    g.close()
    torch.cuda.empty_cache()


def test_spmm_bf16_refuses_row_mapped_graph(ctx):
    rp, ci = random_graph(500, 6, seed=4)
    g = ctx.graph(rp, ci)
    rmap = torch.arange(500, dtype=torch.int32, device="cuda")
    capi._check(ctx.lib.gaib_graph_set_row_map(ctx.h, g.h, rmap.data_ptr(), 500), "gaib_graph_set_row_map")
    x = torch.zeros(500, 16, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(500, 16, device="cuda")
    rc = ctx.lib.gaib_spmm_bf16(ctx.h, g.h, capi.W_MEAN, None, 16, x.data_ptr(), out.data_ptr(), 0)
    assert rc == -5, rc  # GAIB_ERR_UNSUPPORTED
    g.close()


# ---- layers with agg_bf16 = 1 -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lctx():
    return L.init(0)


@pytest.fixture
def bf16_on(lctx):
    lctx.set_option("agg_bf16", 1)
    assert lctx.get_option("agg_bf16") == 1
    yield lctx
    lctx.set_option("agg_bf16", 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def feat(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def cora():
    rp = np.fromfile(GOLD / "cora" / "graph.vertex.bin", np.int64)
    ci = np.fromfile(GOLD / "cora" / "graph.edge.bin", np.uint32)
    return rp, ci


def dense_ops(rp, ci, n, gcn):
    """(A_hat, its transpose) in fp64: GCN's symmetric normalisation over the graph with self loops, SAGE's row mean"""
    deg = np.diff(rp).astype(np.float64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    A = np.zeros((n, n))
    if gcn:
        vd = 1.0 / np.sqrt(deg)
        np.add.at(A, (rows, ci), vd[rows] * vd[ci.astype(np.int64)])
    else:
        np.add.at(A, (rows, ci), 1.0 / deg[rows])
    return A, A.T


def within(got, want, bound, fp32_scale, what):
    """|got - want| <= 1.01 u_bf16 * bound (one bf16 rounding of the gathered table, in absolute values) + fp32 rounding"""
    got = got.astype(np.float64)
    tol = 1.01 * U_BF16 * bound + ELEM_RTOL * fp32_scale + ELEM_FLOOR * np.abs(want).max()
    bad = np.abs(got - want) > tol
    assert not bad.any(), f"{what}: {bad.sum()} entries outside the bound, worst {np.max(np.abs(got - want) - tol):.3g}"
    # and the rounding shows: the bf16 path is not the fp32 one
    return float(np.abs(got - want).max())


def run_layer(kind, level, n, din, dout, g_d, x, gin, constant=False):
    ld = L.Layer(kind, level, n, din, dout, g_d, False)
    xd = dev(x)
    if level == 0:
        ld.set_feat_in(xd)
        if constant:
            ld.set_input_constant(True)
    else:
        ld.write(L.FEAT_IN, xd)
    out = torch.empty(n, dout, device="cuda")
    ld.forward(out)
    if constant:
        ld.forward(out)  # the kept aggregate
    ld.write(L.GRAD_IN, dev(gin))
    grad_out = torch.zeros(n, din, device="cuda") if level > 0 else None
    ld.backward(out, grad_out)
    L.sync()
    res = dict(out=out.cpu().numpy(), W=ld.tensor(L.W_NEIGH, (din, dout)).cpu().numpy().astype(np.float64),
               Wg=ld.tensor(L.W_NEIGH_GRAD, (din, dout)).cpu().numpy(),
               go=grad_out.cpu().numpy() if grad_out is not None else None)
    if kind == L.SAGE:
        res["Ws"] = ld.tensor(L.W_SELF, (din, dout)).cpu().numpy().astype(np.float64)
        res["Wsg"] = ld.tensor(L.W_SELF_GRAD, (din, dout)).cpu().numpy()
    ld.close()
    return res


@pytest.mark.parametrize("arch", ["gcn", "sage"])
@pytest.mark.parametrize("din,dout,level", [(1433, 16, 0), (16, 7, 1), (128, 128, 1), (64, 128, 0), (128, 128, 0)])
def test_layers_with_bf16_tables(bf16_on, arch, din, dout, level):
    gcn = arch == "gcn"
    rp, ci = cora()
    g_o = orc.Graph(rp, ci).add_selfloop() if gcn else orc.Graph(rp, ci)
    rp_l, ci_l = np.asarray(g_o.rowptr, np.int64), np.asarray(g_o.colidx, np.uint32)
    g_d = L.LGraph.from_host(rp, ci, add_selfloop=gcn)
    n = 2708
    x = feat(n, din, 1).astype(np.float64).astype(np.float32)
    gin = feat(n, dout, 2)
    A, At = dense_ops(rp_l, ci_l, n, gcn)
    for constant in ([False, True] if level == 0 else [False]):
        r = run_layer(L.GCN if gcn else L.SAGE, level, n, din, dout, g_d, x, gin, constant)
        X, G, W = x.astype(np.float64), gin.astype(np.float64), r["W"]
        aX, aG, aW = np.abs(X), np.abs(G), np.abs(W)
        Ws = r.get("Ws")
        # forward: out = A X W (+ X Ws); one rounded table (X, or the product X W) on the neighbour path
        want = A @ X @ W + (X @ Ws if Ws is not None else 0)
        bound = A @ aX @ aW
        selfs = aX @ np.abs(Ws) if Ws is not None else 0
        within(r["out"], want, bound, bound + selfs, f"{arch} forward")
        # weight gradient: (A X)^T G -- the rounded table is X (kept aggregate) or G (aggregated in backward)
        within(r["Wg"], X.T @ At @ G, aX.T @ At @ aG, aX.T @ At @ aG, f"{arch} W_neigh_grad")
        if Ws is not None:
            within(r["Wsg"], X.T @ G, 0.0, aX.T @ aG, "sage W_self_grad")
        if level > 0:
            want_go = At @ G @ W.T + (G @ Ws.T if Ws is not None else 0)
            bound_go = At @ aG @ aW.T
            within(r["go"], want_go, bound_go, bound_go + (aG @ np.abs(Ws).T if Ws is not None else 0), f"{arch} grad_out")
    g_d.close()


def test_option_off_is_bit_identical_to_never_set(lctx):
    rp, ci = cora()
    n, din, dout = 2708, 64, 128
    x, gin = feat(n, din, 5), feat(n, dout, 6)
    outs = []
    for step in range(2):
        g_d = L.LGraph.from_host(rp, ci, add_selfloop=True)
        outs.append(run_layer(L.GCN, 1, n, din, dout, g_d, x, gin))
        g_d.close()
        if step == 0:  # on and off again
            lctx.set_option("agg_bf16", 1)
            lctx.set_option("agg_bf16", 0)
    for k in ("out", "Wg", "go"):
        assert np.array_equal(outs[0][k].view(np.uint32), outs[1][k].view(np.uint32)), k


HALO_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from graphaibench_amd import layers as L
from util import random_graph
c = L.init(0)
c.set_option("agg_bf16", 1)
rp, ci = random_graph(400, 6, seed=1)
g = L.LGraph.from_host(rp, ci, add_selfloop=False)
h = c.graph(np.zeros(401, np.int64), np.zeros(0, np.uint32), ncols=1)
g.set_halo(h, lambda n, p: None, lambda n: 0)
ld = L.Layer(L.SAGE, 1, 400, 32, 16, g, False)
ld.write(L.FEAT_IN, torch.randn(400, 32, device="cuda"))
ld.forward(torch.empty(400, 16, device="cuda"))
L.sync()
print("NOT REFUSED")
"""


def test_halo_graph_refuses_bf16_tables(tmp_path):
    """a partitioned (halo) graph with agg_bf16 fails loudly, no silent fp32 path (in a process of its own: it exits)"""
    script = tmp_path / "halo_bf16.py"
    script.write_text(HALO_SCRIPT)
    r = subprocess.run([sys.executable, str(script), str(ROOT)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "NOT REFUSED" not in r.stdout, r.stdout[-1000:] + r.stderr[-1000:]
    assert "agg_bf16" in r.stderr and "halo" in r.stderr, r.stderr[-1000:]


# ---- the trainer --------------------------------------------------------------------------------------------------------
def make_dataset(tmp_path, feat_len=96, seed=0):
    """$DATASET_PATH/cora/: cora's topology and labels with synthetic learnable features"""
    d = tmp_path / "data" / "cora"
    d.mkdir(parents=True)
    for f in ("graph.vertex.bin", "graph.edge.bin", "graph.vlabel.bin"):
        shutil.copyfile(GOLD / "cora" / f, d / f)
    meta = (GOLD / "cora" / "graph.meta.txt").read_text().split()
    meta[7] = str(feat_len)
    (d / "graph.meta.txt").write_text("\n".join(meta) + "\n")
    rng = np.random.default_rng(seed)
    labels = np.fromfile(d / "graph.vlabel.bin", np.uint8)
    x = rng.standard_normal((2708, feat_len)).astype(np.float32) * 0.5
    x[np.arange(2708), labels.astype(int) % feat_len] += 1.5
    x.tofile(d / "graph.feats.bin")
    return str(tmp_path / "data") + "/"


@pytest.mark.parametrize("arch,epoch_graph", [("gcn", "1"), ("sage", "0")])
def test_trainer_with_bf16_tables(tmp_path, arch, epoch_graph):
    root = make_dataset(tmp_path)
    exe = ROOT / "bin" / f"gpu_train_{arch}"
    assert exe.exists(), "run graphaibench_amd.build"
    cmd = [str(exe), "cora", "20", "2", "softmax", "64", "0", "0", "0.01", "2", "0", "4", "0"]
    runs = {}
    for dt in ("fp32", "bf16"):
        env = dict(os.environ, DATASET_PATH=root, GAIB_AGG_DTYPE=dt, GAIB_EPOCH_GRAPH=epoch_graph, GAIB_EPOCH_LOSSES="1")
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert f"aggregation tables: {dt}" in r.stdout
        if epoch_graph == "1":
            assert "recorded as HIP graphs" in r.stderr
        m = re.search(r"epoch_losses ([0-9eE.+\- ]+)", r.stdout + r.stderr)
        losses = [float(v) for v in m.group(1).split()] if m else [float(a) for a in re.findall(r"train_loss ([0-9.]+)", r.stdout)]
        assert len(losses) == 20, losses
        runs[dt] = losses
    b, f = runs["bf16"], runs["fp32"]
    assert b[-1] < b[0] * 0.9, b
    assert abs(b[-1] - f[-1]) <= 0.02 * f[-1], (b[-1], f[-1])
