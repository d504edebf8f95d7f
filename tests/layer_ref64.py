"""The three graph convolution layers in fp64 (numpy, host only), written from their mathematics and not from the control flow
of host/layers.cpp, and the operands of the exact layer tests (tests/test_layer_ref_cpu.py, tests/test_gpu_layers_exact.py,
tests/test_gpu_gat_layers64.py).

    D(X) = X * m * s          m the feature-dropout mask READ FROM THE LAYER, s = 1 / (1 - rate); D(X) = X without dropout
    G'   = G * [out > 0]      where the layer has its activation (relu), else G

    GCN    out = act(A D(X) W)                     dW = (A D(X))^T G'                      grad_out = (A^T G' W^T) * m * s
    SAGE   out = act(M D(X) W_n + D(X) W_s)        dW_n = (M D(X))^T G',  dW_s = D(X)^T G'  grad_out = (M^T G' W_n^T + G' W_s^T) * m * s
    GAT    h = D(X) W;  (out, d_h, alpha gradients) = gat_ref64.gat_ref64 on h and G'      dW = D(X)^T d_h,  grad_out = d_h W^T * m * s

A, M and M^T are poison.weights64's kinds "gcn", "mean" and "mean_t" through exact.agg_ref64 (A^T = A: the graph is symmetric).
Level 0 has no grad_out.

On exact.regular_graph every weight of A and M is a power of two, the smallest 2^-10 (exact.UNIT).  With integer X, G, W, W_s, the
dropout rate 0.5 (s = 2 exactly) and relu, every term of every product and aggregation of a GCN or SAGE layer is an integer number
of units, and while the sum of the ABSOLUTE terms stays below 2^24 units every partial sum in any order is exact in fp32:
a correct layer returns the bits of the fp64 reference, forward and backward.  layer_operands asserts that bound from the data,
for any mask (|D(X)| <= s |X|, |G'| <= |G|).

The bf16 routes (option agg_bf16) cast every aggregated table to bf16.  X, D(X) and G' are bf16 values; a table that is itself a
product -- D(X) W where din > dout, G' W^T where din < dout -- is not, and is rounded to nearest even.  `round_xw` / `round_gwt`
apply that rounding in the reference (bf16_round): such a cell is compared with the reference built on the rounded table.

GAT is not exact (exp) and has two jumps: relu' where an output crosses 0 and leaky-relu' where a score does.  The GAT comparisons
run every backward on the reference's output, and hold the alpha gradients to the nearest reference that takes either slope on the
scores lying within their own fp32 error bound of 0 (undecided_slopes, nearest_alpha_reference)."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import exact as E
import gat_ref64 as R

# the branch matrix of the exact tests: (din, dout); din > dout, din < dout, din == dout (128 and 256: the packed gradient tables)
SHAPES = ((128, 47), (300, 16), (47, 128), (100, 128), (64, 64), (128, 128), (256, 256), (256, 128))
KINDS = ("gcn", "sage")
RATE = 0.5
CELLS = [(kind, din, dout, level, act, drop) for kind in KINDS for din, dout in SHAPES for level in (0, 1)
         for act in (False, True) for drop in (0.0, RATE)]
# the trainer's sequence and the routes: one shape per width relation
RELATION_SHAPES = ((128, 47), (100, 128), (128, 128))


def graph_of(kind: str):
    """GCN runs on the regular graph with its self loops, SAGE on the one without"""
    return E.regular_graph(selfloop=(kind == "gcn"))


def scale_of(rate: float) -> float:
    """the layer's feat_scale = 1 / (1 - rate), taken in fp32 as the constructor does (2 exactly at 0.5)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate))) if rate > 0 else 1.0


def dropped(x, mask=None, scale: float = 1.0) -> np.ndarray:
    x = np.asarray(x, np.float64)
    return x if mask is None else x * np.asarray(mask, np.float64) * scale


def bf16_round(a) -> np.ndarray:
    """fp64 -> bf16 to nearest even -> fp64 (through fp32, which holds the integers of these tests exactly)"""
    import torch

    a32 = np.asarray(a, np.float32)
    assert np.array_equal(a32.astype(np.float64), a)
    return torch.from_numpy(a32).to(torch.bfloat16).to(torch.float64).numpy()


def _back(grad, out, act):
    grad = np.asarray(grad, np.float64)
    return np.where(out > 0, grad, 0.0) if act else grad


def _ident(a):
    return a


def gcn_ref64(G, x, W, grad=None, act=True, level=1, mask=None, scale=1.0, round_xw=None, round_gwt=None) -> SimpleNamespace:
    """the GCN layer on the graph G (exact.regular_graph's record).  grad None: the forward alone"""
    W = np.asarray(W, np.float64)
    dx = dropped(x, mask, scale)
    ax = E.agg_ref64(G, "gcn", dx)
    pre = ax @ W if round_xw is None else E.agg_ref64(G, "gcn", round_xw(dx @ W))
    out = np.maximum(pre, 0.0) if act else pre
    res = SimpleNamespace(out=out, ax=ax, dx=dx, gmask=None, dW=None, dW_self=None, grad_out=None)
    if grad is None:
        return res
    g = _back(grad, out, act)
    res.gmask, res.dW = g, ax.T @ g
    if level > 0:
        res.grad_out = dropped(E.agg_ref64(G, "gcn", (round_gwt or _ident)(g @ W.T)), mask, scale)
    return res


def sage_ref64(G, x, W, W_self, grad=None, act=True, level=1, mask=None, scale=1.0, round_xw=None, round_gwt=None) -> SimpleNamespace:
    """the SAGE layer (mean aggregation + self term)"""
    W, W_self = np.asarray(W, np.float64), np.asarray(W_self, np.float64)
    dx = dropped(x, mask, scale)
    ax = E.agg_ref64(G, "mean", dx)
    pre = (ax @ W if round_xw is None else E.agg_ref64(G, "mean", round_xw(dx @ W))) + dx @ W_self
    out = np.maximum(pre, 0.0) if act else pre
    res = SimpleNamespace(out=out, ax=ax, dx=dx, gmask=None, dW=None, dW_self=None, grad_out=None)
    if grad is None:
        return res
    g = _back(grad, out, act)
    res.gmask, res.dW, res.dW_self = g, ax.T @ g, dx.T @ g
    if level > 0:
        res.grad_out = dropped(E.agg_ref64(G, "mean_t", (round_gwt or _ident)(g @ W.T)) + g @ W_self.T, mask, scale)
    return res


def layer_ref64(kind: str, G, ops, grad=None, act=True, level=1, mask=None, scale=1.0, **rounding) -> SimpleNamespace:
    if kind == "gcn":
        return gcn_ref64(G, ops.x, ops.W, grad, act, level, mask, scale, **rounding)
    return sage_ref64(G, ops.x, ops.W, ops.W_self, grad, act, level, mask, scale, **rounding)


def gat_layer_ref64(rp, ci, x, W, alpha_l, alpha_r, grad, heads, act=True, level=1, mask=None, scale=1.0) -> SimpleNamespace:
    """the GAT layer: h = D(X) W, attention and its backward by gat_ref64.gat_ref64 (d_h is the transposed aggregation alone, the
    reference's semantics), dW = D(X)^T d_h, grad_out = d_h W^T * m * s.  Also t, p, the alpha gradients and their scales."""
    W = np.asarray(W, np.float64)
    dx = dropped(x, mask, scale)
    h = dx @ W
    g = np.asarray(grad, np.float64)
    if act:  # the output does not depend on the gradient: one pass for it, one for the backward on G'
        pre = R.gat_ref64(rp, ci, h, alpha_l, alpha_r, np.zeros_like(h), heads)[2]
        g = _back(g, pre, True)
    t, p, pre, d_h, lg, rg, scale_l, scale_r = R.gat_ref64(rp, ci, h, alpha_l, alpha_r, g, heads)
    out = np.maximum(pre, 0.0) if act else pre
    res = SimpleNamespace(h=h, t=t, p=p, pre=pre, out=out, gmask=g, d_h=d_h, lg=lg, rg=rg, scale_l=scale_l, scale_r=scale_r,
                          dW=dx.T @ d_h, grad_out=None)
    if level > 0:
        res.grad_out = dropped(d_h @ W.T, mask, scale)
    res.undecided = undecided_slopes(rp, ci, dx, W, alpha_l, alpha_r, g, heads, res)
    return res


def undecided_slopes(rp, ci, dx, W, alpha_l, alpha_r, g, heads, ref, eps=0.2) -> list:
    """leaky-relu' jumps at a score of 0, and fp32 cannot tell the sign of a score that is smaller than its own rounding error: a
    (edge, head) whose |t| lies within the first-order error bound of its fp32 evaluation -- h = D(X) W over din terms, the two
    dots over dh terms, their sum: (din + dh + 2) 2^-24 times the sum of the absolute terms, |a_l| . (|D(X)| |W|)[row] +
    |a_r| . (|D(X)| |W|)[col] -- may take either slope in a correct fp32 layer.  Returns, per such (edge, head), the change
    (d alpha_l', d alpha_r') of the alpha gradients when it takes the OTHER slope than the fp64 score's: ge_e = ds_e slope."""
    rows, col = R.rows_of(np.asarray(rp, np.int64)), np.asarray(ci).astype(np.int64)
    n, d = ref.h.shape
    dh, din = d // heads, dx.shape[1]
    gamma = (din + dh + 2) * 2.0 ** -24
    habs = np.abs(dx) @ np.abs(W)
    al, ar = np.abs(np.asarray(alpha_l, np.float64)), np.abs(np.asarray(alpha_r, np.float64))
    found = []
    for k in range(heads):
        sl = slice(k * dh, (k + 1) * dh)
        err = gamma * ((habs[:, sl] @ al[sl])[rows] + (habs[:, sl] @ ar[sl])[col])
        t, p = ref.t[:, k], ref.p[:, k]
        for e in np.nonzero(np.abs(t) <= err)[0]:
            hk = ref.h[:, sl]
            dp = (g[rows][:, sl] * hk[col]).sum(1)
            dot = (p * dp)[rp[rows[e]]:rp[rows[e] + 1]].sum()
            ds = p[e] * (dp[e] - dot)
            delta = ds * ((eps - 1.0) if t[e] > 0 else (1.0 - eps))
            dl, dr = np.zeros(d), np.zeros(d)
            dl[sl], dr[sl] = delta * hk[rows[e]], delta * hk[col[e]]
            found.append((dl, dr))
    return found


def nearest_alpha_reference(ref, lg, rg) -> SimpleNamespace:
    """among the admissible references -- every choice of slope on the undecided (edge, head) pairs (undecided_slopes) -- one near
    (lg, rg) in units of the scales: pairs are flipped one at a time while that brings the reference closer (a search that stops
    short only makes the comparison stricter: whatever it returns is admissible).  (lg, rg, scale_l, scale_r, flipped, undecided)
    for test_gpu_gat_extremes.alpha_close."""
    und = ref.undecided
    dist = lambda l, r: max(R.alpha_ratio(lg, l, ref.scale_l), R.alpha_ratio(rg, r, ref.scale_r))  # noqa: E731
    l, r, taken = ref.lg.copy(), ref.rg.copy(), set()
    best = dist(l, r)
    improved = True
    while improved:
        improved = False
        for i, (dl, dr) in enumerate(und):
            sign = -1.0 if i in taken else 1.0
            d = dist(l + sign * dl, r + sign * dr)
            if d < best:
                l, r, best, improved = l + sign * dl, r + sign * dr, d, True
                taken ^= {i}
    return SimpleNamespace(lg=l, rg=r, scale_l=ref.scale_l, scale_r=ref.scale_r, flipped=len(taken), undecided=len(und))


# ---- the operands of the exact layers -------------------------------------------------------------------------------------------------
BOUNDS = ("A.D(X)", "D(X).W", "out", "dW", "dW_self", "G'.W^T", "grad_out")


def layer_bounds(kind: str, G, x, g, W, W_self, scale: float) -> dict:
    """the sum of the absolute terms of every product and aggregation of the layer, in units of exact.UNIT, for ANY mask and any
    relu pattern: |D(X)| <= s |X|, |G'| <= |G|.  Products and aggregations of non-negative operands associate, so one evaluation
    order bounds them all (A (|X| |W|) = (A |X|) |W|)."""
    fwd, bwd = ("gcn", "gcn") if kind == "gcn" else ("mean", "mean_t")
    a, ag = scale * np.abs(x).astype(np.float64), np.abs(g).astype(np.float64)
    aw, aws = np.abs(W).astype(np.float64), np.abs(W_self).astype(np.float64)
    sage = kind == "sage"
    Aa = E.agg_ref64(G, fwd, a)
    gwt = ag @ aw.T
    tops = {
        "A.D(X)": Aa.max(),
        "D(X).W": (a @ aw).max() if not sage else max((a @ aw).max(), (a @ aws).max()),
        "out": (Aa @ aw + (a @ aws if sage else 0.0)).max(),
        "dW": (Aa.T @ ag).max(),
        "dW_self": (a.T @ ag).max() if sage else 0.0,
        "G'.W^T": gwt.max(),
        "grad_out": scale * (E.agg_ref64(G, bwd, gwt) + (ag @ aws.T if sage else 0.0)).max(),
    }
    return {k: float(v) / E.UNIT for k, v in tops.items()}


@functools.lru_cache(maxsize=None)
def layer_operands(kind: str, din: int, dout: int, drop: float = 0.0, seed: int = 0) -> SimpleNamespace:
    """x [nv x din], g [nv x dout], W and W_self [din x dout]: integers in [-3, 3], float32, read-only.  Asserted from the data:
    every bound of layer_bounds is below 2^24 units of exact.UNIT.  A case that does not fit gets a narrower range of G (never a
    wider bound); `grange` is the range it ended with.  The second gradient g2 (the trainer's second step) obeys the same bound."""
    G = graph_of(kind)
    scale = scale_of(drop)
    rng = np.random.default_rng([seed, din, dout, KINDS.index(kind), G.nv])
    x = E._ints(rng, (G.nv, din), -3, 3)
    W, W_self = E._ints(rng, (din, dout), -3, 3), E._ints(rng, (din, dout), -3, 3)
    for grange in (3, 2, 1):
        g, g2 = E._ints(rng, (G.nv, dout), -grange, grange), E._ints(rng, (G.nv, dout), -grange, grange)
        tops = layer_bounds(kind, G, x, np.maximum(np.abs(g), np.abs(g2)), W, W_self, scale)
        if max(tops.values()) < E.LIMIT:
            break
    worst = max(tops, key=tops.get)
    assert tops[worst] < E.LIMIT, f"{kind} {din} -> {dout} drop {drop}: {worst} may reach {tops[worst]:.0f} >= 2^24 units"
    for a in (x, g, g2, W, W_self):
        a.setflags(write=False)
    return SimpleNamespace(kind=kind, din=din, dout=dout, drop=drop, scale=scale, x=x, g=g, g2=g2, W=W, W_self=W_self, tops=tops,
                           top=tops[worst], grange=grange)


# ---- the comparison: equality of the fp64 reference cast to fp32 ---------------------------------------------------------------------
def mismatch(got, ref64, what: str = ""):
    """None where `got` (float32, numpy or torch) equals the fp64 reference cast to fp32 -- which must hold it exactly: an integer
    number of units below 2^24 of them --, else a message with the number of differing entries and the first of them"""
    import torch

    ref64 = np.asarray(ref64, np.float64)
    E.assert_dyadic(ref64)
    want = torch.from_numpy(ref64.astype(np.float32))
    assert np.array_equal(want.numpy().astype(np.float64), ref64)
    got = got.detach().cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    if got.dtype != torch.float32 or tuple(got.shape) != tuple(want.shape):
        return f"{what}: {got.dtype} {tuple(got.shape)}, expected float32 {tuple(want.shape)}"
    if torch.equal(got, want):
        return None
    bad = torch.nonzero(~(got == want))  # (a NaN differs from everything)
    at = tuple(int(v) for v in bad[0])
    return f"{what}: {len(bad)} of {want.numel()} entries differ, first at {at}: {float(got[at])!r}, reference {float(want[at])!r}"


def assert_same(got, ref64, what: str = "") -> None:
    msg = mismatch(got, ref64, what)
    assert msg is None, msg


# ---- GAT: the graph and the cases ---------------------------------------------------------------------------------------------------
GAT_N = 1500
GAT_SHAPES = ((100, 64), (64, 64), (32, 64), (64, 8))
GAT_CELLS = [(din, dout, heads, act, level, drop) for din, dout in GAT_SHAPES for heads in (1, 8) for act in (False, True)
             for level in (0, 1) for drop in (0.0, RATE)]


@functools.lru_cache(maxsize=None)
def gat_graph():
    """1500 vertices with self loops (gat_ref64's helpers): a power-law graph whose vertex 0 is a hub row of more than four
    64-edge chunks with a short last chunk.  Returns (rowptr int64, colidx uint32)."""
    rp, ci = R._with_selfloops(GAT_N, *R.random_graph(GAT_N, 8, seed=0x6A7, power_law=True, hub_deg=300))
    deg = np.diff(rp)
    assert deg[R.HUB] > 4 * R.CHUNK and deg[R.HUB] % R.CHUNK != 0 and (deg >= 1).all() and deg[1:].max() < deg[R.HUB]
    rows = R.rows_of(rp)
    assert int((rows == ci).sum()) == GAT_N
    for a in (rp, ci):
        a.setflags(write=False)
    return rp, ci


def glorot(rng, din: int, dout: int) -> np.ndarray:
    """uniform in the Glorot range +-sqrt(6 / (din + dout))"""
    r = np.sqrt(6.0 / (din + dout))
    return rng.uniform(-r, r, (din, dout)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gat_operands(din: int, dout: int, heads: int, seed: int = 0) -> SimpleNamespace:
    """N(0,1) features and gradient, Glorot-range W and attention vectors, float32, read-only"""
    rng = np.random.default_rng([seed, din, dout, heads, 0x6A7])
    x = rng.standard_normal((GAT_N, din)).astype(np.float32)
    g = rng.standard_normal((GAT_N, dout)).astype(np.float32)
    W = glorot(rng, din, dout)
    al, ar = glorot(rng, dout, 1).ravel(), glorot(rng, dout, 1).ravel()
    for a in (x, g, W, al, ar):
        a.setflags(write=False)
    return SimpleNamespace(din=din, dout=dout, heads=heads, x=x, g=g, W=W, al=al, ar=ar)


def seeded_mask(shape, seed: int, rate: float = RATE) -> np.ndarray:
    """a 0 / 1 mask for the host-only tests (the GPU tests read the layer's own)"""
    return (np.random.default_rng([seed, 0xD509]).random(shape) >= rate).astype(np.uint8)


def oracle_gat_layer(rp, ci, x32, W, al, ar, grad, heads, act, level, mask_out=None):
    """the fp32 oracle's operators composed into the GAT layer on the input x32 (= D(X) in fp32), head by head, as
    tests/test_gpu_layers.py::test_gat_layer_8_heads composes them: (out, dW, grad_out, alpha_l', alpha_r').  mask_out: the
    output whose sign masks the gradient instead of the oracle's own (G' jumps where an output crosses 0: an output of 2e-7
    that fp32 takes to the other side changes whole rows of the backward, so the GAT comparisons run every backward on the
    REFERENCE's output, as tests/test_gpu_layers.py::test_gat_attention_dropout does)"""
    from oracle import binding as orc

    g_o = orc.Graph(rp, ci)
    h = orc.matmul(x32, W)
    agg, temp, _, norm = orc.gat_aggregate_mh(g_o, h, al, ar, heads)
    out = orc.relu(agg) if act else agg
    g = orc.d_relu(np.array(grad, np.float32), out if mask_out is None else np.asarray(mask_out, np.float32)) if act else np.array(grad, np.float32)
    T, _, _, lg, rg = orc.gat_d_aggregate_mh(g_o, h, g, norm, temp, heads)
    return SimpleNamespace(out=out, d_h=T, dW=orc.matmul(x32, T, True, False), grad_out=orc.matmul(T, W, False, True) if level > 0 else None,
                           lg=lg, rg=rg, p=norm.reshape(-1, heads), temp=temp.reshape(-1, heads))


def gat_distances(o, ref, mask=None, scale: float = 1.0) -> dict:
    """the fp32 oracle's own distances from the fp64 reference on one cell, as tests/test_gpu_gat_extremes.py's Case takes them:
    element-wise (util.elem_err, default floor) for out, dW and grad_out, the alpha gradients in units of their scale against the
    nearest admissible reference (nearest_alpha_reference).  The oracle ran on D(X); its grad_out gets the mask and the scale here."""
    from util import elem_err

    near = nearest_alpha_reference(ref, o.lg, o.rg)
    d = {"out": elem_err(o.out, ref.out), "dW": elem_err(o.dW, ref.dW),
         "alpha": max(R.alpha_ratio(o.lg, near.lg, ref.scale_l), R.alpha_ratio(o.rg, near.rg, ref.scale_r))}
    if ref.grad_out is not None:
        d["grad_out"] = elem_err(dropped(o.grad_out, mask, scale), ref.grad_out)
    return d
