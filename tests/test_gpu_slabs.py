"""GPU suite: the column slabs of the one-row-per-wave aggregation (dispatch_vec, csrc/spmm_kernels.h).

One launch covers 256 lanes' worth of columns (128 lanes at 16 B); a wider row is cut into column slabs, each a launch
of its own over the row's edge list with in / out moved by the slab's first column c0.  Everything that a kernel derives
from a lane's column has to count from the WHOLE row's column 0 there -- with per-head edge weights the head is
(c0 + column in the slab) / dh, and slab cuts fall inside heads.

Every case is compared with the CPU oracle at the suite's own bars: rows up to the heavy threshold bit for bit (same CSR
order, separate multiply and add), rows above it -- summed by 16 waves in another order -- within assert_close at
LONG_SUM_FLOOR (util.py gives the reason for that floor).  Per-head references are built head by head from the
single-head oracle, with independently drawn weights per head: a wrong head is an O(1) error.
"""
import numpy as np
import pytest
import torch

from graphaibench_amd import capi
from oracle import binding as orc
from util import LONG_SUM_FLOOR, assert_close, random_graph

pytestmark = pytest.mark.gpu
PREFILL = 9.0
KINDS = ["gcn", "mean", "mean_t", "edge", "edge_t"]
KIND_ID = {"gcn": capi.W_GCN, "mean": capi.W_MEAN, "mean_t": capi.W_MEAN_T, "edge": capi.W_EDGE, "edge_t": capi.W_EDGE_T}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class SlabGraph:
    """1300 power-law vertices, a 1200-edge hub in row 0 (the heavy kernel at the default threshold) and three empty rows at
    the end; the oracle's results per width, computed once and handed out read-only"""

    def __init__(self, ctx):
        rp, ci = random_graph(1300, 8, 41, power_law=True, hub_deg=1200)
        rp = np.concatenate([rp, [rp[-1]] * 3])  # three empty rows at the end (square graph: columns stay valid)
        self.g_o = orc.Graph(rp, ci)
        self.g_d = ctx.graph(rp, ci.view(np.int32))
        self.n, self.ne = self.g_o.nv, self.g_o.ne
        self.deg = np.diff(rp)
        assert self.deg[0] > 1024 and self.deg[1:].max() <= 1024 and (self.deg[1:] > 32).sum() > 20
        rng = np.random.default_rng(5)
        self.ew = rng.random(self.ne).astype(np.float32)
        # every kind as explicit edge weights, formed the way the oracle's aggregators form them (checked below): what the
        # accumulate leg's same-order reference needs
        rows = np.repeat(np.arange(self.n), self.deg)
        vd = self.g_o.vertex_data()
        inv = lambda dg: (1.0 / dg.astype(np.float32).astype(np.float64)).astype(np.float32)
        self.w = {"gcn": vd[rows] * vd[ci], "mean": inv(self.deg[rows]), "mean_t": inv(self.deg[ci]), "edge": self.ew,
                  "edge_t": orc.symmetric_csr_transpose(self.g_o, self.ew)}
        x8 = self.x(8)
        for kind in KINDS:
            assert np.array_equal(bits(orc.spmm_edge(self.g_o, self.w[kind], x8)), bits(self.named(kind, x8))), kind
        # the same graph with one leading edge per row, of weight 1, to an extra vertex whose feature row is PREFILL: the
        # oracle then sums ((0 + 1 * PREFILL) + t0) + t1 ..., which is the kernel's order when it continues a pre-filled row
        self.g_pre = orc.Graph(rp + np.arange(self.n + 1), np.insert(ci, rp[:-1], self.n))
        self.w_pre = {k: np.insert(w, rp[:-1], np.float32(1.0)) for k, w in self.w.items()}
        self._x, self._plain, self._acc, self._mh = {}, {}, {}, {}

    def x(self, d):
        return np.random.default_rng(1000 + d).standard_normal((self.n, d)).astype(np.float32)

    def named(self, kind, x):
        if kind == "gcn":
            return orc.gcn_aggregate(self.g_o, x)
        if kind == "mean":
            return orc.sage_aggregate(self.g_o, x)
        if kind == "mean_t":
            return orc.sage_d_aggregate(self.g_o, x)
        if kind == "edge":
            return orc.spmm_edge(self.g_o, self.ew, x)
        return orc.spmm_edge(self.g_o, orc.symmetric_csr_transpose(self.g_o, self.ew), x)

    def plain(self, kind, d):
        if (kind, d) not in self._plain:
            self._plain[kind, d] = self.named(kind, self.x(d))
            self._plain[kind, d].setflags(write=False)
        return self._plain[kind, d]

    def continued(self, kind, d):
        """relu(PREFILL-filled row + aggregation), the prefill first in the sum"""
        if (kind, d) not in self._acc:
            xp = np.concatenate([self.x(d), np.full((1, d), PREFILL, np.float32)])
            s = orc.spmm_edge(self.g_pre, self.w_pre[kind], xp)
            self._acc[kind, d] = np.where(s > 0, s, np.float32(0))
            self._acc[kind, d].setflags(write=False)
        return self._acc[kind, d]

    def heads(self, heads, dh):
        """(ew [ne][heads], {kind: want}): columns [k * dh, (k + 1) * dh) are the single-head oracle on head k's weights"""
        if (heads, dh) not in self._mh:
            x = self.x(heads * dh)
            ew = torch.rand(self.ne, heads, generator=torch.Generator().manual_seed(heads * 1000 + dh)).numpy()
            want = {"edge": np.empty_like(x), "edge_t": np.empty_like(x)}
            for k in range(heads):
                xk, wk = np.ascontiguousarray(x[:, k * dh:(k + 1) * dh]), np.ascontiguousarray(ew[:, k])
                want["edge"][:, k * dh:(k + 1) * dh] = orc.spmm_edge(self.g_o, wk, xk)
                want["edge_t"][:, k * dh:(k + 1) * dh] = orc.spmm_edge(self.g_o, orc.symmetric_csr_transpose(self.g_o, wk), xk)
            for w in want.values():
                w.setflags(write=False)
            self._mh[heads, dh] = (ew, want)
        return self._mh[heads, dh]

    def check(self, got, want, thr, what):
        got = got.cpu().numpy()
        light = self.deg <= thr
        assert np.array_equal(bits(got[light]), bits(want[light])), f"{what}: rows of at most {thr} edges must be bit-exact"
        assert_close(got[~light], want[~light], f"{what}, rows above {thr} edges", floor=LONG_SUM_FLOOR)


@pytest.fixture(scope="module")
def G(ctx):
    g = SlabGraph(ctx)
    yield g
    g.g_d.close()


def run_single_head(ctx, G, d, thr=1024, carve=False):
    """every weight kind at width d: plainly into a pre-filled buffer, then continuing a pre-filled buffer with relu on store"""

    def table(fill=None):  # carve: one float into a larger buffer -- base pointers aligned to 4 bytes only
        buf = torch.empty(G.n * d + (1 if carve else 0), device="cuda")
        t = buf[1:] if carve else buf
        assert t.data_ptr() % 8 == (4 if carve else 0)
        return t.view(G.n, d) if fill is None else t.fill_(fill).view(G.n, d)

    x = table()
    x.copy_(torch.from_numpy(G.x(d)))
    ew = torch.from_numpy(G.ew).cuda()
    for kind in KINDS:
        w = ew if kind in ("edge", "edge_t") else None
        out = ctx.spmm(G.g_d, KIND_ID[kind], x, table(PREFILL), edge_w=w)
        G.check(out, G.plain(kind, d), thr, f"{kind} d={d}")
        out = ctx.spmm(G.g_d, KIND_ID[kind], x, table(PREFILL), edge_w=w, accumulate=True, relu=True)
        G.check(out, G.continued(kind, d), thr, f"{kind} d={d} accumulate + relu")


# ---- a: single-head slabs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [257, 513, 769,  # 4-byte lanes: 256 + 1, 256 + 256 + 1, three full slabs + 1
                               514,            # 8-byte lanes: 512 + 2
                               516, 1028])     # 16-byte lanes: 512 + 4, 512 + 512 + 4
def test_single_head_slabs(ctx, G, d):
    run_single_head(ctx, G, d)


def test_single_head_slabs_many_heavy_rows(ctx, G):
    """heavy threshold 32: many rows take the 16-wave kernel, in every slab"""
    ctx.set_option("spmm_heavy_threshold", 32)
    try:
        run_single_head(ctx, G, 516, thr=32)
    finally:
        ctx.set_option("spmm_heavy_threshold", 1024)


def test_single_head_slabs_base_pointers_aligned_to_4_bytes(ctx, G):
    """x and out one float into their buffers: 4-byte lanes whatever the width -- 516 columns in three slabs"""
    run_single_head(ctx, G, 516, carve=True)


# ---- b: per-head weights across slabs --------------------------------------------------------------------------------
def run_heads(ctx, G, heads, dh, thr):
    ew, want = G.heads(heads, dh)
    x, ewd = torch.from_numpy(G.x(heads * dh)).cuda(), torch.from_numpy(ew).cuda()
    outs = []
    for kind in ("edge", "edge_t"):
        out = torch.full((G.n, heads * dh), PREFILL, device="cuda")
        ctx.spmm(G.g_d, KIND_ID[kind], x, out, edge_w=ewd, heads=heads)
        G.check(out, want[kind], thr, f"{kind} {heads} heads x {dh}")
        outs.append(out)
    return outs


@pytest.mark.parametrize("thr", [1024, 32])
@pytest.mark.parametrize("heads,dh", [(2, 129),   # 258 columns, 4-byte lanes: c0 = 256 inside head 1
                                      (8, 65),    # 520, 4-byte lanes: slabs 256 / 256 / 8, both cuts inside a head
                                      (4, 130),   # 520, 8-byte lanes: c0 = 512 inside head 3
                                      (8, 128),   # 1024, 16-byte lanes: c0 = 512 on a head boundary (the 8 x 128 GAT layer)
                                      (16, 64),   # 1024
                                      (3, 200)])  # 600, 16-byte lanes: c0 = 512 inside head 2
def test_per_head_weights_across_slabs(ctx, G, heads, dh, thr):
    ctx.set_option("spmm_heavy_threshold", thr)
    try:
        run_heads(ctx, G, heads, dh, thr)
    finally:
        ctx.set_option("spmm_heavy_threshold", 1024)


@pytest.mark.parametrize("thr", [1024, 32])
def test_per_head_weights_forced_4_byte_lanes(ctx, G, thr):
    """8 heads x 40 = 320 columns: two slabs under spmm_variant = 1, one launch of 16-byte lanes by default -- the same sum
    per element in the same order, so the same bits"""
    ctx.set_option("spmm_heavy_threshold", thr)
    try:
        ctx.set_option("spmm_variant", 1)
        try:
            forced = run_heads(ctx, G, 8, 40, thr)
        finally:
            ctx.set_option("spmm_variant", 0)
        auto = run_heads(ctx, G, 8, 40, thr)
    finally:
        ctx.set_option("spmm_heavy_threshold", 1024)
    for a, b in zip(forced, auto):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- c: the suite's own checks at slab widths (their bodies, called with shapes their parameter lists stop short of) ------
import test_gpu_bf16 as bf16_suite  # noqa: E402
import test_gpu_classes as class_suite  # noqa: E402
import test_gpu_fuzz as fuzz_suite  # noqa: E402
import test_gpu_ops as ops_suite  # noqa: E402


@pytest.mark.parametrize("d,heads,hub", [(1024, 8, 1700), (520, 8, 0)])
def test_gat_multi_head_across_slabs(ctx, d, heads, hub):
    """test_gpu_ops.test_gat_multi_head -- the staged GAT chain against the multi-head oracle -- at 8 x 128 and 8 x 65 columns:
    its W_EDGE / W_EDGE_T aggregations take a second / third slab (gat_scores, sddmm, gat_softmax_bwd_alpha and
    edge_transpose are width-generic and pass as they are)"""
    ops_suite.test_gat_multi_head(ctx, d, heads, hub)


@pytest.mark.parametrize("d", [301, 522, 1028])  # part_vec: 256 + 45 (4-byte lanes), 512 + 10 (8-byte), 1024 + 4 (16-byte, four tiles)
@pytest.mark.parametrize("kind,name", class_suite.KINDS)
def test_class_aggregation_across_slabs(ctx, d, kind, name):
    """test_gpu_classes.test_class_aggregation_matches_oracle_and_round3_split at the fp32 partition launcher's slab widths"""
    class_suite.test_class_aggregation_matches_oracle_and_round3_split(ctx, d, kind, name)


def test_spmm_bf16_slabs_accumulate_and_relu_together(ctx):
    """dispatch_bf16's slabs: test_gpu_bf16.test_spmm_bf16_bit_identical runs 513 and 1024 columns with every weight kind under
    accumulate OR relu -- here both at once (that file's bar: the bits of the fp32 call on the widened table), on light rows, a
    hub row and empty rows"""
    rp, ci = random_graph(1300, 8, seed=4, power_law=True, hub_deg=1200)
    rp = np.concatenate([rp, [rp[-1]] * 3])
    g = ctx.graph(rp, ci)
    try:
        n = bf16_suite.check_identity(ctx, g, len(rp) - 1, [513, 1024], flag_sets=((True, True),))
    finally:
        g.close()
    assert n == 2 * len(bf16_suite.KINDS)


def test_short_seeded_sweep_of_fuzz_spmm():
    """scripts/fuzz_spmm.py (widths up to 1028, per-head weights up to 8 x 129) the way test_gpu_fuzz runs its sweeps"""
    fuzz_suite.test_short_seeded_sweep("fuzz_spmm.py", [])
