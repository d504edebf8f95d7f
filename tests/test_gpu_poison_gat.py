"""GPU suite, the GAT kernels in the leak direction only (tests/poison.py has the method): NaN in four rows of h -- rows 0 and
nv - 1 and two other light rows, none of them adjacent to a hub -- on the poison graph with self loops.  The dependent set is
where tests/gat_ref64.py, run on the poisoned input, is not finite (a row's whole softmax once one of its scores is NaN; for
grad_out the columns such a row leads to).  Everywhere else out, the attention array, the row statistics, the per-edge arrays of
the staged pieces and grad_out keep the clean run's bits.  What the kernels write AT dependent entries is printed (pytest -s)
and recorded in LEDGER 23, not asserted: the reduce's S > 0 guard legitimately turns a NaN row into zeros.  The alpha gradients
are global sums and are not part of this file.

Paths: the staged pieces (light rows and the workgroup-per-row launches at spmm_heavy_threshold 100), the one sweep in fp32,
on bf16 tables, under attention dropout 0.3, and on rows wider than 128 columns (gat_fused_wide), at (64, 8) and (256, 8).
The clean run is held to the fp64 reference with assert_close (LONG_SUM_FLOOR on the rows above 100 edges alone, as the other
GAT files do where a graph has hubs)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gat_ref64 as R
import poison as P
from graphaibench_amd import capi
from util import LONG_SUM_FLOOR, assert_close

pytestmark = pytest.mark.gpu

DEFAULTS = dict(gat_fused_fwd=-1, gat_fused_bwd=-1, gat_fused_wide=0, spmm_heavy_threshold=1024)
SHAPES = [(64, 8), (256, 8)]
SEED = 0x5EED0002
RATE = 0.3


@pytest.fixture
def knobs(ctx):
    """every option a test may set goes back to its default afterwards"""
    try:
        yield ctx
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


def bf16_round(a):
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


class Case:
    """the inputs at one (len, heads), clean and poisoned, the fp64 reference of both, the dependent sets"""

    def __init__(self, ctx, d, heads, bf=False, mask=None, scale=1.0):
        G = self.G = P.graph(True)
        P.check_graph(G)
        self.d, self.heads = d, heads
        rng = np.random.default_rng(100 + d)
        h, grad = (rng.standard_normal((G.nv, d)).astype(np.float32) for _ in range(2))
        if bf:
            h, grad = bf16_round(h), bf16_round(grad)
        self.al, self.ar = ((0.2 * rng.standard_normal(d)).astype(np.float32) for _ in range(2))
        self.h, self.grad = h, grad
        self.hp = h.copy()
        self.hp[list(P.quiet_rows(True))] = np.nan
        keys = ("t", "p", "out", "grad_out")
        self.ref = SimpleNamespace(**dict(zip(keys, R.gat_ref64(G.rp, G.ci, h, self.al, self.ar, grad, heads, mask=mask, scale=scale)[:4])))
        with np.errstate(invalid="ignore"):
            bad = dict(zip(keys, (~np.isfinite(a) for a in R.gat_ref64(G.rp, G.ci, self.hp, self.al, self.ar, grad, heads)[:4])))
        row_bad = np.zeros((G.nv, heads), bool)
        np.logical_or.at(row_bad, G.rows, bad["p"])
        self.dep = dict(t=bad["t"], p=bad["p"], s=bad["p"], out=bad["out"], grad_out=bad["grad_out"],
                        stats=np.repeat(row_bad[:, :, None], 2, 2), dp=np.repeat(np.isin(G.ci, P.quiet_rows(True))[:, None], heads, 1))
        for k, m in self.dep.items():
            P.shares(m, f"GAT {d} x {heads} {k}")
        assert not self.dep["out"][list(G.hubs)].any()  # (no hub row depends on the poison)
        self.long = np.nonzero(G.deg > P.HEAVY)[0]
        self.g = ctx.graph(G.rp.copy(), G.ci.view(np.int32).copy())

    def close_to(self, got, want, what, edges=False):
        """assert_close, with LONG_SUM_FLOOR on the rows above 100 edges (edges: on their edges) alone"""
        long = np.isin(self.G.rows, self.long) if edges else np.isin(np.arange(self.G.nv), self.long)
        assert_close(got[~long], want[~long], what)
        assert_close(got[long], want[long], what + ", rows above 100 edges", floor=LONG_SUM_FLOOR)


LEDGER = {}


def tally(path, name, dirty, dep):
    """what a kernel wrote at the dependent entries: counted, printed, not asserted"""
    v = dirty[dep]
    c = LEDGER.setdefault((path, name), np.zeros(4, np.int64))
    c += [int(np.isnan(v).sum()), int(np.isinf(v).sum()), int((v == 0).sum()), int((np.isfinite(v) & (v != 0)).sum())]
    print(f"    at dependent entries, {path} {name}: NaN {c[0]}, inf {c[1]}, zero {c[2]}, other finite {c[3]}")


def both(path, c, run, names):
    """run(h table as numpy) -> host arrays by name; clean against poisoned"""
    clean, dirty = run(c.h), run(c.hp)
    for k in names:
        P.compare(clean[k], dirty[k], c.dep[k], None, f"{path} {c.d} x {c.heads} {k}")
        tally(f"{path} ({c.d}, {c.heads})", k, dirty[k], c.dep[k])
    return clean


@pytest.mark.parametrize("heavy", [1024, P.HEAVY])
@pytest.mark.parametrize("d,heads", SHAPES)
def test_staged_pieces(knobs, d, heads, heavy):
    ctx = knobs
    ctx.set_option("spmm_heavy_threshold", heavy)
    c = Case(ctx, d, heads)
    G, ne = c.G, c.G.ne
    al, ar, grad = P.table(c.al), P.table(c.ar), P.table(c.grad)

    def run(h):
        hd = P.table(h)
        t, s, p, dp = (P.Out(ne, heads) for _ in range(4))
        out, go = P.Out(G.nv, d), P.Out(G.nv, d)
        ctx.gat_scores(c.g, hd, al, ar, t.t, s.t, p.t, heads=heads)
        ctx.spmm(c.g, capi.W_EDGE, hd, out.t, edge_w=p.t, heads=heads)
        ctx.sddmm(c.g, grad, hd, dp.t, heads=heads)
        ctx.spmm(c.g, capi.W_EDGE_T, grad, go.t, edge_w=p.t, heads=heads)
        return {k: o.host(f"staged {k}") for k, o in dict(t=t, s=s, p=p, out=out, dp=dp, grad_out=go).items()}

    try:
        clean = both(f"staged, threshold {heavy}", c, run, ("t", "s", "p", "out", "dp", "grad_out"))
        assert_close(clean["t"], c.ref.t, "temp")
        c.close_to(clean["p"], c.ref.p, "attention", edges=True)
        c.close_to(clean["out"], c.ref.out, "out")
        c.close_to(clean["grad_out"], c.ref.grad_out, "grad_out")
    finally:
        c.g.close()


def library_mask(ctx, ne, heads):
    """the mask gaib_dropout draws over an [ne * heads] array under SEED (what the _drop calls use)"""
    ones = torch.ones(ne * heads, device="cuda")
    m = torch.empty(ne * heads, dtype=torch.uint8, device="cuda")
    ctx.dropout(ones, m, torch.empty_like(ones), RATE, SEED)
    ctx.sync()
    return m.cpu().numpy().reshape(ne, heads)


@pytest.mark.parametrize("form", ["fp32", "bf16", "dropout"])
@pytest.mark.parametrize("d,heads", SHAPES)
def test_one_sweep(knobs, d, heads, form):
    """forward, then backward from its output and statistics; (256, 8) is the wide form, one sweep per column slab"""
    ctx = knobs
    ctx.set_option("gat_fused_fwd", 1)
    ctx.set_option("gat_fused_bwd", 1)
    ctx.set_option("gat_fused_wide", 1 if d > 128 else 0)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(RATE)))
    mask = library_mask(ctx, P.graph(True).ne, heads) if form == "dropout" else None
    c = Case(ctx, d, heads, bf=form == "bf16", mask=mask, scale=scale)
    G = c.G
    dt = torch.bfloat16 if form == "bf16" else None
    al, ar, grad = P.table(c.al), P.table(c.ar), P.table(c.grad, dt)

    def run(h):
        hd = P.table(h, dt)
        out, stats, go, lg, rg = P.Out(G.nv, d), P.Out(G.nv, heads, 2), P.Out(G.nv, d), P.Out(d), P.Out(d)
        if form == "fp32":
            assert ctx.gat_forward_fused(c.g, hd, al, ar, out.t, stats.t, heads=heads)
            assert ctx.gat_backward_fused(c.g, hd, grad, out.t, al, ar, None, go.t, lg.t, rg.t, heads=heads, row_stats=stats.t)
        elif form == "bf16":
            assert ctx.gat_forward_fused_bf16(c.g, hd, al, ar, out.t, stats.t, heads=heads)
            assert ctx.gat_backward_fused_bf16(c.g, hd, grad, out.t, al, ar, go.t, lg.t, rg.t, stats.t, heads=heads)
        else:
            assert ctx.gat_forward_fused_drop(c.g, hd, al, ar, out.t, stats.t, RATE, SEED, scale=scale, heads=heads)
            assert ctx.gat_backward_fused_drop(c.g, hd, grad, out.t, al, ar, go.t, lg.t, rg.t, stats.t, RATE, SEED, scale=scale, heads=heads)
        ctx.sync()
        lg.host("alpha_l gradient"), rg.host("alpha_r gradient")  # (written, their tails untouched; the values are global sums)
        return dict(out=out.host("out"), stats=stats.host("row statistics"), grad_out=go.host("grad_out"))

    try:
        clean = both(f"one sweep {form}" + (", column slabs" if d > 128 else ""), c, run, ("out", "stats", "grad_out"))
        c.close_to(clean["out"], c.ref.out, "out")
        c.close_to(clean["grad_out"], c.ref.grad_out, "grad_out")
        # the attention formed again from the statistics (row max, 1 / row sum), as the backward does
        st = clean["stats"].astype(np.float64)
        t = c.ref.t
        p = np.exp(np.where(t > 0, t, 0.2 * t) - st[G.rows, :, 0]) * st[G.rows, :, 1]
        c.close_to(p, c.ref.p, "attention from the statistics", edges=True)
    finally:
        c.g.close()
