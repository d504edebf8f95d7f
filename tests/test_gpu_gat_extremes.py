"""GPU suite, the GAT kernels where the rest of the suite never takes them (tests/gat_ref64.py has the inputs): pre-activation
scores of +-80 and past +-200, rows whose scores rise or fall along the row (the online softmax rescales at every step, or
never), scores of exactly 0 (the jump of leaky-relu'), rows whose scores are all equal, rows without an edge, rows of exactly
64 and 65 edges, a hub row of four full chunks and a short one, and (row, head) pairs whose every edge is dropped.

Everything is held to the fp64 reference gat_ref64.gat_ref64:
  * out, the attention and grad_out through assert_close's two metrics with rtol = max(1e-4, twice the fp32 oracle's own
    element-wise distance from fp64 on the same inputs) and the default floor -- LONG_SUM_FLOOR on the hub row alone, as the
    other GAT tests do where a graph has a hub (sums of hundreds of terms taken in another order);
  * the alpha gradients in units of the magnitude their sums went through (scale_l, scale_r of the reference):
    max_j |got - ref| / scale <= max(twice the oracle's same ratio, 16 * 2^-24).  The second term: the kernels form p again
    with the fast exponential, whose argument product x * log2(e) rounds at 2^-24 relative, so the result carries |x| * 2^-24;
    an edge with |s - M| > 16 weighs less than 1.2e-7 of its row.
Each test prints the measured figures (pytest -s).

Measured on an MI355X, the worst over the shapes and launch options of a family -- out / attention / grad_out element-wise,
alpha gradients in units of the scale; every alpha figure is below 6.4e-8 against the bound of 9.5e-7:
    family     oracle                        staged                        one sweep, from the statistics
    wide       7.5e-5 7.1e-6 1.6e-5 2.8e-8   4.3e-5 6.4e-6 8.2e-6 2.0e-8   3.8e-5 5.4e-6 7.9e-6 2.1e-8
    asc        2.1e-5 2.1e-5 4.3e-5 4.6e-9   8.3e-6 7.8e-6 8.3e-6 1.2e-8   7.2e-6 1.2e-5 1.5e-5 1.3e-8
    desc       1.8e-5 1.7e-5 1.4e-4 1.1e-8   1.1e-5 1.1e-5 2.0e-5 7.8e-9   2.4e-5 2.1e-5 5.4e-5 1.1e-8
    underflow  3.5e-4 1.8e-5 8.9e-5 3.1e-8   3.6e-4 1.2e-5 2.7e-5 2.2e-8   3.2e-4 1.8e-5 2.6e-5 2.6e-8
    uniform    1.5e-6 4.5e-8 8.5e-6 2.3e-8   1.5e-6 4.5e-8 3.1e-6 1.3e-8   2.4e-6 2.3e-6 1.7e-6 1.4e-8
    zero       1.6e-6 4.5e-8 8.7e-6 2.6e-8   1.6e-6 4.5e-8 2.6e-6 7.6e-9   1.6e-6 4.5e-8 2.1e-6 1.1e-8
    benign     1.1e-5 9.0e-7 6.9e-6 1.6e-8   4.2e-6 4.3e-7 1.7e-6 1.6e-8   5.0e-6 6.5e-7 1.7e-6 1.4e-8
(the other paths -- from the attention array, bf16 tables, dropout, column slabs -- lie in the same ranges; LEDGER 21 has them).

What the file notices, tried on builds with one line of csrc/gat_kernels.h changed: GAT_NEG = -INFINITY (NaN wherever a lane
group of a short chunk holds no edge), the reduce's 1 / S without its S > 0 guard (NaN on the rows without an edge), the row
maximum of the reduce replaced by the first chunk's (inf on `asc`, whose last chunk lies 100 above its first), and
leaky-relu' taken as 1 at a score of exactly 0 on the column side (`zero` alone sees it: alpha_r's gradient five times too
large).  The same change on the row side is invisible by construction: a row's ds sum to 0."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gat_ref64 as R
from graphaibench_amd import capi
from util import ELEM_FLOOR, LONG_SUM_FLOOR, elem_err, rel_err

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
ALPHA_FLOOR = 16 * 2.0 ** -24
SEED = 0x5EED0001
DEFAULTS = dict(gat_fused_fwd=-1, gat_fused_bwd=-1, gat_fused_unroll=4, gat_bwd_pk=0, gat_fused_wide=0, spmm_heavy_threshold=1024)
CASES = [(name, d, heads) for name in R.FAMILIES for d, heads in ((64, 8), (128, 2))]
SWEEP_CASES = [(name, d, heads) for name in R.FAMILIES for d, heads in ((32, 1), (64, 8), (128, 2), (128, 16))]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the families' arrays are read-only)


def filled(*shape):
    return torch.full(shape, SENTINEL, device="cuda")


def host(t, what):
    a = t.cpu().numpy()
    assert np.isfinite(a).all(), f"{what}: not finite"
    assert not (a == SENTINEL).any(), f"{what}: left unwritten"
    return a


@pytest.fixture
def knobs(ctx):
    """every option a test may set goes back to its default afterwards"""
    yield ctx
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)


def close(got, want, o, what, long_rows=()):
    """assert_close's two metrics against fp64 with rtol = max(1e-4, twice o, the oracle's own element-wise distance from fp64
    on these inputs) and the default floor, LONG_SUM_FLOOR on the rows `long_rows` alone.  Returns the element-wise error."""
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64).reshape(want.shape)
    rtol = max(1e-4, 2 * o)
    floor = np.full(want.shape[0], ELEM_FLOOR)
    floor[list(long_rows)] = LONG_SUM_FLOOR
    scale = max(np.abs(want).max(), 1e-30)
    e = float((np.abs(got - want) / (np.abs(want) + (floor / rtol * scale).reshape((-1,) + (1,) * (want.ndim - 1)))).max())
    r = rel_err(got, want)
    print(f"    {what}: element-wise {e:.2e} (oracle {o:.2e}, rtol {rtol:.1e})")
    assert r <= rtol and e <= rtol, f"{what}: norm-wise {r:.3e}, element-wise {e:.3e} (rtol {rtol:.2e}, oracle {o:.3e})"
    return e


def alpha_close(lg, rg, ref, o, what):
    """the alpha gradients in units of scale_l / scale_r: <= max(twice o, the oracle's ratio on these inputs, 16 * 2^-24)"""
    got = max(R.alpha_ratio(lg, ref.lg, ref.scale_l), R.alpha_ratio(rg, ref.rg, ref.scale_r))
    print(f"    {what}: alpha gradients {got:.2e} of the scale (oracle {o:.2e})")
    assert got <= max(2 * o, ALPHA_FLOOR), f"{what}: alpha gradients {got:.3e} of the scale, oracle {o:.3e}, bound {max(2 * o, ALPHA_FLOOR):.3e}"
    return got


class Case:
    """one (family, len, heads) on the device, with its fp64 reference and the oracle's results"""

    def __init__(self, ctx, name, d, heads, ins=None, ref=None, orc_=None):
        self.name, self.d, self.heads = name, d, heads
        self.rp, self.ci, h, al, ar, grad = ins if ins is not None else R.family(name, d, heads)
        self.ref, self.orc = (ref, orc_) if ref is not None else R.family_reference(name, d, heads)
        self.n, self.ne = len(self.rp) - 1, len(self.ci)
        self.rows, self.deg = R.rows_of(self.rp), np.diff(self.rp)
        self.hub_edges = np.arange(self.rp[R.HUB], self.rp[R.HUB + 1])
        self.empty = np.nonzero(self.deg == 0)[0]
        self.h, self.al, self.ar, self.grad = dev(h), dev(al), dev(ar), dev(grad)
        self.g = ctx.graph(self.rp, self.ci.view(np.int32))
        self.what = f"{name} {d}x{heads}"
        # the oracle's own distances from fp64 (it has no dropout: a dropped sweep is given the undropped oracle's figures)
        r, o = self.ref, self.orc
        self.oerr = SimpleNamespace(**{k: elem_err(getattr(o, k), getattr(r, k)) for k in ("out", "p", "grad_out")},
                                    temp=elem_err(o.temp, r.t),
                                    alpha=max(R.alpha_ratio(o.lg, r.lg, r.scale_l), R.alpha_ratio(o.rg, r.rg, r.scale_r)))

    def close(self):
        self.g.close()

    def p_from_stats(self, stats):
        """exp(leaky(t64) - M) * (1 / S) with the kernels' row statistics"""
        st = stats.astype(np.float64)
        t = self.ref.t
        return np.exp(np.where(t > 0, t, 0.2 * t) - st[self.rows, :, 0]) * st[self.rows, :, 1]


@pytest.fixture
def case(knobs):
    """Case(...) on the session's context; the graphs are closed afterwards"""
    made = []

    def make(*a, **k):
        made.append(Case(knobs, *a, **k))
        return made[-1]

    yield make
    for c in made:
        c.close()


# ---- (a) the staged path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heavy", [1024, 100])  # 100: the hub rows take the workgroup-per-row kernels
@pytest.mark.parametrize("name,d,heads", CASES)
def test_staged(knobs, case, name, d, heads, heavy):
    ctx = knobs
    ctx.set_option("spmm_heavy_threshold", heavy)
    c = case(name, d, heads)
    ref, o, n, ne, what = c.ref, c.oerr, c.n, c.ne, f"staged {c.what} heavy {heavy}"
    print(what)
    hub = [R.HUB]
    t, s, p = filled(ne, heads), filled(ne, heads), filled(ne, heads)
    ctx.gat_scores(c.g, c.h, c.al, c.ar, t, s, p, heads=heads)
    close(host(t, "temp"), ref.t, o.temp, what + " temp")
    close(host(p, "norm"), ref.p, o.p, what + " norm", long_rows=c.hub_edges)
    host(s, "scores")
    if name == "zero":
        assert bool((t == 0).all())
    out = filled(n, d)
    ctx.spmm(c.g, capi.W_EDGE, c.h, out, edge_w=p, heads=heads)
    close(host(out, "out"), ref.out, o.out, what + " out", long_rows=hub)
    assert not out[c.empty].any()
    dp = filled(ne, heads)
    ctx.sddmm(c.g, c.grad, c.h, dp, heads=heads)
    hk, gk = (a.cpu().numpy().astype(np.float64).reshape(n, heads, -1) for a in (c.h, c.grad))
    dp64 = (gk[c.rows] * hk[c.ci.astype(np.int64)]).sum(2)
    close(host(dp, "sddmm"), dp64, elem_err(c.orc.dp, dp64), what + " sddmm")
    go = filled(n, d)
    ctx.spmm(c.g, capi.W_EDGE_T, c.grad, go, edge_w=p, heads=heads)
    close(host(go, "grad_out"), ref.grad_out, o.grad_out, what + " grad_out", long_rows=hub)
    forms = {"with temp": dict(temp=t), "one pass": dict(temp=t, grad_rows=c.grad, fwd_out_rows=out),
             "re-formed sign": dict(temp=None, alpha=(c.al, c.ar))}
    for form, kw in forms.items():
        lg, rg, ds = filled(d), filled(d), filled(ne, heads)
        ctx.gat_softmax_bwd_alpha(c.g, c.h, p, dp, kw.pop("temp"), ds, lg, rg, heads=heads, **kw)
        host(ds, "ds")
        alpha_close(host(lg, "alpha_l grad"), host(rg, "alpha_r grad"), ref, o.alpha, f"{what} {form}")


# ---- (b) one sweep, fp32 ------------------------------------------------------------------------------------------------------------
def sweep(ctx, c, rate=None, norm=None, bf=None, seed=SEED):
    """forward, then backward on its output, into sentinel-filled outputs, twice: identical bits.  norm: backward from the
    attention array instead of the statistics; rate: the _drop calls; bf: (h, grad) as bf16 tables, the _bf16 calls"""
    n, d, heads = c.n, c.d, c.heads
    h, grad = bf if bf is not None else (c.h, c.grad)
    sfx = "_bf16" if bf is not None else ""
    runs = []
    for _ in range(2):
        out, stats, go, lg, rg = filled(n, d), filled(n, heads, 2), filled(n, d), filled(d), filled(d)
        if rate is None:
            assert getattr(ctx, "gat_forward_fused" + sfx)(c.g, h, c.al, c.ar, out, stats, heads=heads)
            if bf is None:
                assert ctx.gat_backward_fused(c.g, h, grad, out, c.al, c.ar, norm, go, lg, rg, heads=heads,
                                              row_stats=None if norm is not None else stats)
            else:
                assert ctx.gat_backward_fused_bf16(c.g, h, grad, out, c.al, c.ar, go, lg, rg, stats, heads=heads)
        else:
            scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))
            assert getattr(ctx, "gat_forward_fused_drop" + sfx)(c.g, h, c.al, c.ar, out, stats, rate, seed, scale=scale, heads=heads)
            assert getattr(ctx, "gat_backward_fused_drop" + sfx)(c.g, h, grad, out, c.al, c.ar, go, lg, rg, stats, rate, seed,
                                                                  scale=scale, heads=heads)
        ctx.sync()
        runs.append((out, stats, go, lg, rg))
    for name, a, b in zip(("out", "row_stats", "grad_out", "alpha_l grad", "alpha_r grad"), *runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{c.what}: {name} differs between two runs"
    keys = ("out", "stats", "grad_out", "lg", "rg")
    return SimpleNamespace(dev=dict(zip(keys, runs[0])), **{k: host(t, f"{c.what} {k}") for k, t in zip(keys, runs[0])})


def check_sweep(c, res, what, ref=None, fully_dropped=None):
    ref, o, hub = ref or c.ref, c.oerr, [R.HUB]
    close(res.out, ref.out, o.out, what + " out", long_rows=hub)
    close(res.grad_out, ref.grad_out, o.grad_out, what + " grad_out", long_rows=hub)
    alpha_close(res.lg, res.rg, ref, o.alpha, what)
    if len(c.empty):  # a row without an edge: exact zeros, finite statistics (host() has looked)
        assert not res.out[c.empty].any() and not res.grad_out[c.empty].any(), what
    if fully_dropped is not None:
        rows_, heads_ = fully_dropped
        dh = c.d // c.heads
        for i, k in zip(rows_, heads_):
            assert not res.out[i, k * dh:(k + 1) * dh].any(), (what, i, k)


@pytest.mark.parametrize("name,d,heads", SWEEP_CASES)
def test_one_sweep(knobs, case, name, d, heads):
    ctx = knobs
    ctx.set_option("gat_fused_fwd", 1)
    ctx.set_option("gat_fused_bwd", 1)
    c = case(name, d, heads)
    ref, o = c.ref, c.oerr
    pd = dev(ref.p.astype(np.float32))
    first = None
    for unroll in (4, 8):
        for pk in (0, 1):  # (every head here is at most 16 lanes wide: the packed-math backward applies)
            assert (d // heads) // 4 <= 16
            ctx.set_option("gat_fused_unroll", unroll)
            ctx.set_option("gat_bwd_pk", pk)
            what = f"one sweep {c.what} unroll {unroll} pk {pk}"
            print(what)
            res = sweep(ctx, c)
            check_sweep(c, res, what + " from the statistics")
            live = c.deg > 0
            assert (res.stats[live][:, :, 1] > 0).all()
            p_re = c.p_from_stats(res.stats)
            close(p_re, ref.p, o.p, what + " attention from the statistics", long_rows=c.hub_edges)
            if name in ("uniform", "zero"):
                close(p_re, np.broadcast_to((1.0 / c.deg)[c.rows][:, None], p_re.shape), o.p, what + " 1 / deg", long_rows=c.hub_edges)
            check_sweep(c, sweep(ctx, c, norm=pd), what + " from the attention array")
            if first is None:
                first = res
    signs = ctx.gat_score_signs(c.g, c.h, c.al, c.ar, heads=heads).cpu().numpy().reshape(c.ne, heads).astype(bool)
    if name == "zero":
        assert not signs.any()
    diff = signs != (ref.t > 0)
    assert np.abs(ref.t[diff]).max(initial=0.0) <= 1e-5 * np.abs(ref.t).max()


# ---- (c) bf16 tables ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rounded_case(name, d, heads):
    """the family with h and grad rounded to bf16 on the host (to nearest even), its reference and oracle on the widened values"""
    rp, ci, h, al, ar, grad = R.family(name, d, heads)
    rnd = lambda a: torch.from_numpy(a.copy()).to(torch.bfloat16).to(torch.float32).numpy()  # noqa: E731
    ins = (rp, ci, rnd(h), al, ar, rnd(grad))
    R.check_family(name, *ins[:5], heads)  # the rounded table still is what the family promises
    return ins, R.reference(*ins, heads), R.oracle(*ins, heads)


@pytest.mark.parametrize("d,heads", [(64, 8), (128, 2)])
@pytest.mark.parametrize("name", ["wide", "asc", "zero", "benign"])
def test_bf16_tables(knobs, case, name, d, heads):
    ctx = knobs
    ctx.set_option("gat_fused_fwd", 1)
    ctx.set_option("gat_fused_bwd", 1)
    ins, ref, orc_ = rounded_case(name, d, heads)
    c = case(name, d, heads, ins=ins, ref=ref, orc_=orc_)
    hb, gb = c.h.to(torch.bfloat16), c.grad.to(torch.bfloat16)
    assert torch.equal(hb.float(), c.h) and torch.equal(gb.float(), c.grad)  # exact: the values are bf16's
    what = f"bf16 tables {c.what}"
    print(what)
    wide, narrow = sweep(ctx, c), sweep(ctx, c, bf=(hb, gb))
    for k in wide.dev:
        assert torch.equal(wide.dev[k].view(torch.int32), narrow.dev[k].view(torch.int32)), f"{what}: {k} is not the fp32 call's bits"
    check_sweep(c, narrow, what)
    close(c.p_from_stats(narrow.stats), ref.p, c.oerr.p, what + " attention from the statistics", long_rows=c.hub_edges)


# ---- (d) attention dropout ----------------------------------------------------------------------------------------------------------
def library_mask(ctx, ne, heads, rate, seed):
    """the mask gaib_dropout draws over an [ne * heads] array of ones under `seed` (as tests/test_gpu_gat_drop.py does)"""
    ones = torch.ones(ne * heads, device="cuda")
    m = torch.empty(ne * heads, dtype=torch.uint8, device="cuda")
    ctx.dropout(ones, m, torch.empty_like(ones), rate, seed)
    ctx.sync()
    m = m.cpu().numpy().reshape(ne, heads)
    assert set(np.unique(m)) <= {0, 1} and abs(1.0 - m.mean() - rate) < 5 * np.sqrt(rate * (1 - rate) / m.size)
    return m


def dropped(ctx, c, rate, bf=None):
    """the dropped sweep against the fp64 reference under the library's mask; the fully dropped blocks; the statistics' bits"""
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))
    mask = library_mask(ctx, c.ne, c.heads, rate, SEED)
    kept = np.zeros((c.n, c.heads))
    np.add.at(kept, c.rows, mask)
    gone = np.nonzero((kept == 0) & (c.deg > 0)[:, None])  # (row, head) pairs with edges, all of them dropped
    if rate == 0.9:
        assert len(gone[0]) >= 20, len(gone[0])
    ref = R.reference(c.rp, c.ci, c.h.cpu().numpy(), c.al.cpu().numpy(), c.ar.cpu().numpy(), c.grad.cpu().numpy(), c.heads,
                      mask=mask, scale=scale)
    what = f"dropout {rate} {c.what}" + (" bf16" if bf else "")
    print(f"{what}: {len(gone[0])} (row, head) pairs fully dropped")
    res, plain = sweep(ctx, c, rate=rate, bf=bf), sweep(ctx, c, bf=bf)
    check_sweep(c, res, what, ref=ref, fully_dropped=gone)
    assert torch.equal(res.dev["stats"].view(torch.int32), plain.dev["stats"].view(torch.int32)), what + ": the statistics saw the mask"
    return mask, scale, ref


@pytest.mark.parametrize("rate", [0.3, 0.9])
@pytest.mark.parametrize("name", ["wide", "desc", "benign", "uniform"])
def test_attention_dropout(knobs, case, name, rate):
    ctx = knobs
    ctx.set_option("gat_fused_fwd", 1)
    ctx.set_option("gat_fused_bwd", 1)
    c = case(name, 64, 8)
    mask, scale, ref = dropped(ctx, c, rate)
    if name != "wide":
        return
    # the dropped form of the reference against the staged path: attention, the library's dropout on it, the aggregations, and
    # the softmax backward fed with the masked, rescaled d(out)/d(p)
    d, heads, ne, what = c.d, c.heads, c.ne, f"staged dropout {rate} {c.what}"
    p, pm, dp = filled(ne, heads), filled(ne, heads), filled(ne, heads)
    m = torch.empty(ne * heads, dtype=torch.uint8, device="cuda")
    ctx.gat_scores(c.g, c.h, c.al, c.ar, None, None, p, heads=heads)
    ctx.dropout(p.view(-1), m, pm.view(-1), rate, SEED)
    out, go, lg, rg = filled(c.n, d), filled(c.n, d), filled(d), filled(d)
    ctx.spmm(c.g, capi.W_EDGE, c.h, out, edge_w=pm, heads=heads)
    ctx.spmm(c.g, capi.W_EDGE_T, c.grad, go, edge_w=pm, heads=heads)
    ctx.sddmm(c.g, c.grad, c.h, dp, heads=heads)
    dpm = dp * dev(mask.astype(np.float32) * np.float32(scale))
    ctx.gat_softmax_bwd_alpha(c.g, c.h, p, dpm, None, None, lg, rg, heads=heads, alpha=(c.al, c.ar))
    ctx.sync()
    assert np.array_equal(m.cpu().numpy().reshape(ne, heads), mask)
    close(host(out, "out"), ref.out, c.oerr.out, what + " out", long_rows=[R.HUB])
    close(host(go, "grad_out"), ref.grad_out, c.oerr.grad_out, what + " grad_out", long_rows=[R.HUB])
    alpha_close(host(lg, "alpha_l grad"), host(rg, "alpha_r grad"), ref, c.oerr.alpha, what)


def test_attention_dropout_on_bf16_tables(knobs, case):
    ctx = knobs
    ctx.set_option("gat_fused_fwd", 1)
    ctx.set_option("gat_fused_bwd", 1)
    ins, ref, orc_ = rounded_case("wide", 64, 8)
    c = case("wide", 64, 8, ins=ins, ref=ref, orc_=orc_)
    dropped(ctx, c, 0.9, bf=(c.h.to(torch.bfloat16), c.grad.to(torch.bfloat16)))


# ---- (e) column slabs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide", "asc"])
def test_column_slabs(knobs, case, name):
    ctx = knobs
    ctx.set_option("gat_fused_wide", 1)
    ctx.set_option("gat_fused_fwd", 1)
    ctx.set_option("gat_fused_bwd", 1)
    c = case(name, 256, 8)
    what = f"column slabs {c.what}"
    print(what)
    res = sweep(ctx, c)
    check_sweep(c, res, what)
    close(c.p_from_stats(res.stats), c.ref.p, c.oerr.p, what + " attention from the statistics", long_rows=c.hub_edges)
    dropped(ctx, c, 0.3)
