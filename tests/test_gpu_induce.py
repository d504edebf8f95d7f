"""GPU suite: gaib_graph_induce -- the subgraph a vertex set induces on a graph in HBM, built on the device (csrc/induce.hip) --
with gaib_gather_rows_u8 and the trainer's option sampler_device (GAIB_SAMPLER_DEVICE=1) on top of it.  Pinned against the
reference's own Sampler::generateSubgraph / generate_masked_graph outputs (tests/golden/sampler_*.npz), against the
dictionary construction of tests/test_sampler_cpu.py on rows of every chunk count, and -- through the trainer -- against the
host path's loss curve, string for string.  Every array comparison is exact."""
import os
import re
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from graphaibench_amd import capi, layers as L
from util import random_graph

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
MiB = 1 << 20
ERR_INVALID, ERR_UNSUPPORTED = -1, -5


def _induced(rp, ci, ids):
    """tests/test_sampler_cpu.py's construction: row k = the kept neighbours of ids[k], renumbered, in input order"""
    pos = {int(v): k for k, v in enumerate(ids)}
    rows = []
    for v in ids:
        rows.append([pos[int(c)] for c in ci[rp[v]:rp[v + 1]] if int(c) in pos])
    return rows


def _csr(rows):
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c in r], np.uint32)
    return rp, ci


def _masked(rp, ci, ids):
    """generate_masked_graph: every vertex keeps its row under its own id; dropped vertices' rows are empty"""
    keep = set(int(v) for v in ids)
    return _csr([[int(c) for c in ci[rp[v]:rp[v + 1]] if int(c) in keep] if v in keep else [] for v in range(len(rp) - 1)])


def _arrays(g):
    return g.rowptr().cpu().numpy(), g.colidx().cpu().numpy().view(np.uint32)


def _induce(g, kept, keep_ids=False):
    """(rowptr, colidx, rows) of g.induce as numpy arrays; the induced graph is destroyed"""
    sub, rows = g.induce(np.asarray(kept, np.uint32), keep_ids=keep_ids)
    try:
        rp, ci = _arrays(sub)
        assert sub.nv == len(rp) - 1 and sub.ne == len(ci) == rp[-1] and sub.nc == sub.nv
    finally:
        sub.close()
    return rp, ci, rows.cpu().numpy()


def _golden(tag):
    f = np.load(GOLD / f"sampler_{tag}.npz")
    nvtx, deg, gseed, ntrain, n, seed = (int(v) for v in f["params"])
    rp, ci = random_graph(nvtx, deg, seed=gseed, power_law=True)
    return f, rp, ci, ntrain


# ---- 1, 2: the reference's own outputs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["walk_rebuild", "short_walk", "no_walk"])
def test_induce_matches_reference_subgraph(ctx, tag):
    f, rp, ci, _ = _golden(tag)
    g = capi.Graph(ctx, rp, ci)
    try:
        srp, sci, rows = _induce(g, f["kept"])
        assert np.array_equal(srp, f["sub_rowptr"].astype(np.int64)) and np.array_equal(sci, f["sub_colidx"])
        assert np.array_equal(rows, f["kept"].astype(np.int64))
        # the same list from device memory
        sub, rows_d = g.induce(torch.from_numpy(f["kept"].view(np.int32)).cuda())
        drp, dci = _arrays(sub)
        sub.close()
        assert np.array_equal(drp, srp) and np.array_equal(dci, sci) and np.array_equal(rows_d.cpu().numpy(), rows)
    finally:
        g.close()


@pytest.mark.parametrize("tag", ["walk_rebuild", "short_walk", "no_walk"])
def test_induce_keep_ids_matches_reference_masked_graph(ctx, tag):
    f, rp, ci, ntrain = _golden(tag)
    g = capi.Graph(ctx, rp, ci)
    try:
        mrp, mci, rows = _induce(g, np.arange(ntrain, dtype=np.uint32), keep_ids=True)
        assert len(mrp) == len(rp)  # nv rows under the old ids
        assert np.array_equal(mrp, f["masked_rowptr"].astype(np.int64))
        assert np.uint32(zlib.crc32(mci.tobytes())) == f["masked_colidx_crc"]
        assert np.array_equal(rows, np.arange(ntrain))
    finally:
        g.close()


# ---- 3: rows of every chunk count, bitmap word boundaries --------------------------------------------------------------
HAND_DEGREES = (0, 1, 63, 64, 65, 128, 129)
HAND_IDS = tuple(200 + 2 * k for k in range(len(HAND_DEGREES)))  # even ids, away from the word boundaries 64 / 128


@pytest.fixture(scope="module")
def degree_graph():
    """random_graph(3001, 6, hub_deg=2500) -- nv no multiple of 64, vertex 0 a row of 40 chunks -- with seven rows replaced by
    hand-made ones of full degree 0, 1 (a self loop), 63, 64, 65, 128 and 129"""
    rp, ci = random_graph(3001, 6, seed=17, hub_deg=2500)
    nv = len(rp) - 1
    rng = np.random.default_rng(5)
    rows = [list(ci[rp[v]:rp[v + 1]]) for v in range(nv)]
    for v, d in zip(HAND_IDS, HAND_DEGREES):
        rows[v] = [v] if d == 1 else sorted(int(c) for c in rng.choice(nv, d, replace=False))
    rp, ci = _csr(rows)
    return rp, ci, _kept_sets(rp, ci)


def _kept_sets(rp, ci):
    nv = len(rp) - 1
    rng = np.random.default_rng(8)
    sets = {"all": np.arange(nv), "even": np.arange(0, nv, 2)}
    sets["word_edges"] = np.unique(np.concatenate([[63, 64, 127, 128, nv - 1], rng.choice(nv, 300, replace=False)]))
    picked, blocked = set(), set()  # no two members adjacent (in either direction)
    for v in rng.permutation(nv):
        v = int(v)
        nbrs = set(int(c) for c in ci[rp[v]:rp[v + 1]]) - {v}
        if v in blocked or nbrs & picked:
            continue
        picked.add(v)
        blocked |= nbrs
    sets["independent"] = np.array(sorted(picked))
    sets["hub"] = np.array([0])
    return sets


@pytest.mark.parametrize("which", ["all", "even", "word_edges", "independent", "hub"])
@pytest.mark.parametrize("keep_ids", [False, True])
def test_induce_degrees_and_word_boundaries(ctx, degree_graph, which, keep_ids):
    rp, ci, sets = degree_graph
    nv = len(rp) - 1
    assert nv % 64 != 0
    kept = sets[which]
    deg = np.diff(rp)
    # the classes the test is about occur among the rows it walks (a generator change must not empty it)
    if which in ("all", "even"):
        assert set(HAND_DEGREES) <= set(int(d) for d in deg[kept]), sorted(set(deg[kept]))
        assert np.array_equal(deg[list(HAND_IDS)], HAND_DEGREES)
    if which in ("all", "even", "hub"):
        assert deg[0] >= 2500 and kept[0] == 0  # a row of 40 chunks
    if which == "word_edges":
        assert {63, 64, 127, 128, nv - 1} <= set(int(v) for v in kept)
    if which == "independent":
        assert len(kept) > 300
    g = capi.Graph(ctx, rp, ci)
    try:
        got_rp, got_ci, rows = _induce(g, kept, keep_ids=keep_ids)
    finally:
        g.close()
    want_rp, want_ci = _masked(rp, ci, kept) if keep_ids else _csr(_induced(rp, ci, kept))
    assert np.array_equal(got_rp, want_rp) and np.array_equal(got_ci, want_ci)
    assert np.array_equal(rows, kept)
    if which == "all" and not keep_ids:
        assert np.array_equal(got_rp, rp) and np.array_equal(got_ci, ci)
    if which == "independent":
        assert got_rp[-1] == (1 if HAND_IDS[1] in kept else 0)  # only a self loop can survive


# ---- 4: the cached bitmap from call to call ----------------------------------------------------------------------------
def test_induce_workspace_reuse_and_invalid_lists(ctx, degree_graph):
    rp, ci, _ = degree_graph
    nv = len(rp) - 1
    rng = np.random.default_rng(3)
    perm = rng.permutation(nv)
    A, B = np.sort(perm[:1200]), np.sort(perm[1200:2500])
    assert not set(A) & set(B)
    want_a, want_b = _csr(_induced(rp, ci, A)), _csr(_induced(rp, ci, B))
    g = capi.Graph(ctx, rp, ci)
    try:
        first = _induce(g, A)
        second = _induce(g, B)
        third = _induce(g, A)
        for x, y in zip(first, third):
            assert np.array_equal(x, y)
        assert np.array_equal(first[0], want_a[0]) and np.array_equal(first[1], want_a[1])
        assert np.array_equal(second[0], want_b[0]) and np.array_equal(second[1], want_b[1])
        dup = np.concatenate([A[:500], A[499:]])
        desc = A.copy()
        desc[[700, 701]] = desc[[701, 700]]
        over = np.concatenate([A[A < nv - 1], [nv]])
        for bad in (dup, desc, over, np.array([2 ** 32 - 1], np.uint32)):
            for keep_ids in (False, True):
                with pytest.raises(capi.GaibError, match=rf"status {ERR_INVALID}\)"):
                    g.induce(bad.astype(np.uint32), keep_ids=keep_ids)
            after = _induce(g, B)  # the next valid call is correct
            assert np.array_equal(after[0], want_b[0]) and np.array_equal(after[1], want_b[1])
        with pytest.raises(capi.GaibError, match=rf"status {ERR_INVALID}\)"):  # more ids than vertices
            g.induce(np.arange(nv + 1, dtype=np.uint32))
        again = _induce(g, A)
        assert np.array_equal(again[0], want_a[0]) and np.array_equal(again[1], want_a[1])
    finally:
        g.close()


# ---- 5: edge cases and refusals -----------------------------------------------------------------------------------------
def test_induce_edge_cases_and_refusals(ctx, degree_graph):
    rp, ci, _ = degree_graph
    nv = len(rp) - 1
    g = capi.Graph(ctx, rp, ci)
    rect = capi.Graph(ctx, rp, ci, ncols=nv + 5)
    try:
        erp, eci, rows = _induce(g, np.zeros(0, np.uint32))
        assert np.array_equal(erp, [0]) and len(eci) == 0 and len(rows) == 0
        erp, eci, _ = _induce(g, np.zeros(0, np.uint32), keep_ids=True)
        assert np.array_equal(erp, np.zeros(nv + 1, np.int64)) and len(eci) == 0
        for keep_ids in (False, True):  # every vertex kept: g's own CSR in both modes
            arp, aci, rows = _induce(g, np.arange(nv), keep_ids=keep_ids)
            assert np.array_equal(arp, rp) and np.array_equal(aci, ci) and np.array_equal(rows, np.arange(nv))
        with pytest.raises(capi.GaibError, match=rf"status {ERR_UNSUPPORTED}\)"):
            rect.induce(np.arange(10, dtype=np.uint32))
    finally:
        rect.close()
    # inside a recording the call is refused; the recording goes on and replays
    s = capi.Context(0)
    s.own_stream()
    x = torch.randn(nv, 16, device="cuda")
    y_eager, y_rec = torch.empty_like(x), torch.zeros_like(x)
    ex = None
    try:
        g.compute_vertex_data()
        s.spmm(g, capi.W_GCN, x, y_eager)  # once call by call: the lazily built tables exist
        s.sync()
        torch.cuda.synchronize()
        s.capture_begin()
        with pytest.raises(capi.GaibError, match="gaib_capture_begin/end"):
            _with_ctx(g, s).induce(np.arange(10, dtype=np.uint32))
        s.spmm(g, capi.W_GCN, x, y_rec)
        ex = s.capture_end()
        ex.launch()
        s.sync()
        assert torch.equal(y_rec, y_eager)
        sub, _ = _with_ctx(g, s).induce(np.arange(10, dtype=np.uint32))  # and outside it the call works on that context
        want = _csr(_induced(rp, ci, np.arange(10)))
        got = _arrays(sub)
        sub.close()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        if ex is not None:
            ex.close()
        s.close()
        g.close()


def _with_ctx(g, c):
    """a non-owning view of graph g whose calls go through context c"""
    v = capi.Graph.__new__(capi.Graph)
    v.lib, v.ctx, v.h = g.lib, c, g.h
    v.close = lambda: None
    return v


# ---- 6: everything downstream accepts the induced graph ----------------------------------------------------------------
def test_induced_graph_runs_downstream_bit_equal():
    ctx = L.init(0)
    rp0, ci0 = random_graph(4000, 10, seed=9, power_law=True)
    full0 = capi.Graph(ctx, rp0, ci0)
    full = full0.add_selfloop()
    full0.close()
    rp, ci = _arrays(full)
    kept = np.sort(np.random.default_rng(2).choice(4000, 1500, replace=False))
    n = len(kept)
    a, _ = full.induce(kept)
    full.close()
    hrp, hci = _csr(_induced(rp, ci, kept))
    b = capi.Graph(ctx, hrp, hci)
    assert np.array_equal(_arrays(a)[0], hrp) and np.array_equal(_arrays(a)[1], hci)
    for g in (a, b):
        g.compute_vertex_data()
    assert torch.equal(a.vertex_data(), b.vertex_data())
    torch.manual_seed(4)
    for d in (16, 128):
        x = torch.randn(n, d, device="cuda")
        for kind in (capi.W_GCN, capi.W_MEAN):
            ya, yb = torch.empty_like(x), torch.empty_like(x)
            ctx.spmm(a, kind, x, ya)
            ctx.spmm(b, kind, x, yb)
            ctx.sync()
            assert torch.equal(ya, yb), (d, kind)
    # a GAT layer of 1 head x 16 columns, forward and backward: the lazily built tables (edge chunks, reverse-edge
    # permutation) of an adopted induced graph
    d = 16
    x, grad = torch.randn(n, d, device="cuda"), torch.randn(n, d, device="cuda")
    res, layers, graphs = [], [], []
    for g in (a, b):
        lg = L.LGraph.adopt(g)
        layer = L.Layer(L.GAT, 1, n, d, d, lg, True)
        layer.set_heads(1)
        if layers:  # the same parameters in both layers
            for which, shape in ((L.W_NEIGH, (d, d)), (L.ALPHA_L, (d,)), (L.ALPHA_R, (d,))):
                layer.write(which, layers[0].tensor(which, shape))
        out, go = torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")
        layer.write(L.FEAT_IN, x)
        layer.forward(out)
        layer.write(L.GRAD_IN, grad)
        layer.backward(out, go)
        L.sync()
        res.append((out, go, layer.tensor(L.W_NEIGH_GRAD, (d, d)), layer.tensor(L.ALPHA_LGRAD, (d,)),
                    layer.tensor(L.ALPHA_RGRAD, (d,))))
        layers.append(layer)
        graphs.append(lg)
    try:
        for ta, tb in zip(*res):
            assert torch.isfinite(ta).all() and torch.equal(ta, tb)
        assert res[0][0].abs().max() > 0 and res[0][1].abs().max() > 0
    finally:
        for layer in layers:
            layer.close()
        for lg in graphs:
            lg.close()


# ---- 7: byte rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 7, 16])
def test_gather_rows_u8(ctx, width):
    n_in, n_idx = 1000, 777
    gen = torch.Generator().manual_seed(width)
    idx = torch.randint(0, n_in, (n_idx,), generator=gen)
    idx[0], idx[1], idx[-1] = 0, n_in - 1, n_in - 1
    buf_in = torch.randint(0, 256, (n_in * width + 8,), dtype=torch.uint8, generator=gen).cuda()
    buf_out = torch.full((n_idx * width + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    x = buf_in[1:1 + n_in * width].view(n_in, width)      # odd base addresses on both sides
    out = buf_out[3:3 + n_idx * width].view(n_idx, width)
    assert x.data_ptr() % 2 == 1 and out.data_ptr() % 2 == 1
    ctx.gather_rows_u8(idx.cuda(), x, out)
    ctx.sync()
    assert torch.equal(out.cpu(), x.cpu()[idx])
    assert (buf_out[:3] == 0xAB).all() and (buf_out[3 + n_idx * width:] == 0xAB).all()  # nothing outside the rows
    ctx.gather_rows_u8(idx[:0].cuda(), x, out)  # no rows: nothing to do


# ---- 8: memory --------------------------------------------------------------------------------------------------------------
def _free_bytes(ctx):
    ctx.sync()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_induce_releases_its_device_memory(ctx):
    """tests/test_gpu_lifecycle.py's method.  The graph has 2^25 vertices (all but the first 200 000 isolated), so that its
    membership bitmap and prefix directory (4 MiB + 2 MiB) are above the tolerance, like one leaked induced graph."""
    nv, n_live = 1 << 25, 200_000
    rp, ci = random_graph(n_live, 10, seed=6)
    rowptr = torch.full((nv + 1,), int(rp[-1]), dtype=torch.int64, device="cuda")
    rowptr[:n_live + 1] = torch.from_numpy(rp).cuda()
    colidx = torch.from_numpy(ci.view(np.int32)).cuda()
    kept = torch.arange(0, n_live, 2, dtype=torch.int32, device="cuda")

    def rounds(k):
        g = capi.Graph(ctx, rowptr, colidx)
        before = g.device_bytes()
        for _ in range(k):
            sub, rows = g.induce(kept)
            assert sub.nv == n_live // 2 and sub.ne > 100_000
            sub.close()
        assert g.device_bytes() - before == (nv // 64) * 8 + (nv // 64 + 1) * 4  # the cached arrays are counted
        g.close()

    rounds(1)  # the context's workspace and the caches of torch's allocator reach their size
    base = _free_bytes(ctx)
    rounds(40)
    lost = base - _free_bytes(ctx)
    assert lost <= 4 * MiB, f"{lost / MiB:.1f} MiB not returned after 40 induce / destroy rounds and gaib_graph_destroy"


# ---- 9: the trainer ---------------------------------------------------------------------------------------------------------
def _sampling_dataset(tmp_path):
    from test_gpu_driver import make_dataset

    root, *_ = make_dataset(tmp_path)
    meta = (tmp_path / "data" / "cora" / "graph.meta.txt").read_text().split()
    meta[10:13] = ["0", "1500", "1500"]  # a training range large enough to sample from
    (tmp_path / "data" / "cora" / "graph.meta.txt").write_text("\n".join(meta) + "\n")
    return root


def _train(arch, root, **env):
    exe = ROOT / "bin" / f"gpu_train_{arch}"
    assert exe.exists(), "run graphaibench_amd.build"
    cmd = [str(exe), "cora", "12", "3", "softmax", "16", "0", "0", "0.02", "2", "600", "50", "0"]
    base = {k: v for k, v in os.environ.items() if k != "GAIB_SAMPLER_DEVICE"}
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                          env=dict(base, DATASET_PATH=root, GAIB_EPOCH_LOSSES="1", **env))


@pytest.mark.parametrize("arch", ["gcn", "sage", "gat"])
def test_trainer_device_sampler_reproduces_host_loss_curve(tmp_path, arch):
    root = _sampling_dataset(tmp_path)
    host = _train(arch, root, GAIB_EPOCH_TIMES="0")
    assert host.returncode == 0, host.stdout[-2000:] + host.stderr[-2000:]
    dev = _train(arch, root, GAIB_SAMPLER_DEVICE="1", GAIB_EPOCH_TIMES="0")
    assert dev.returncode == 0, dev.stdout[-2000:] + dev.stderr[-2000:]
    lines = []
    for r in (host, dev):
        got = re.findall(r"^\[gaib prof\] (?:epoch_losses|epoch_accs) .*$", r.stdout, re.M)
        assert len(got) == 2 and len(got[0].split()) == 3 + 12, r.stdout[-2000:]
        lines.append(got)
    assert lines[0] == lines[1], (lines[0], lines[1])
    assert "subgraphs: built on the device" in dev.stdout and "built on the device" not in host.stdout
    for r in (host, dev):  # the in-trainer measurement: one figure per epoch, both settings
        timing = re.findall(r"^\[gaib prof\] subgraph_seconds (.*)$", r.stdout, re.M)
        assert len(timing) == 1 and len(timing[0].split()) == 12, r.stdout[-2000:]
    assert "subgraph_seconds" not in _train(arch, root).stdout  # nothing is timed (or waited for) unless asked


def test_trainer_refuses_an_unknown_sampler_device_value(tmp_path):
    root = _sampling_dataset(tmp_path)
    r = _train("gcn", root, GAIB_SAMPLER_DEVICE="2")
    assert r.returncode != 0 and "GAIB_SAMPLER_DEVICE=2" in r.stderr and "0 or 1" in r.stderr
