"""The GAT aggregation and its backward in fp64 (numpy, host only), and the input families of the extreme-score tests
(tests/test_gat_extremes_cpu.py, tests/test_gpu_gat_extremes.py): score ranges of +-80 and beyond, rows whose scores rise or
fall along the row, rows whose scores are all equal or all exactly 0, rows without an edge, rows of exactly 64 and 65 edges
(the one-sweep kernels' chunk boundary), and a hub row of four full chunks and a short one.

The alpha gradients are sums that cancel (exactly, on the `uniform` and `zero` families), so the reference also returns the
magnitude of the summed terms; an implementation is judged in units of that magnitude (alpha_ratio)."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from util import csr_from_pairs, random_graph

CHUNK = 64  # edges per chunk of the one-sweep kernels
FAMILIES = ("wide", "asc", "desc", "underflow", "uniform", "zero", "benign")
SHAPES = ((32, 1), (64, 8), (128, 2))


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def gat_ref64(rowptr, colidx, h, alpha_l, alpha_r, grad, heads, eps=0.2, mask=None, scale=1.0):
    """Per head k over the columns [k dh, (k + 1) dh):
        t_e = a_l.h[row_e] + a_r.h[col_e],  s = leaky_eps(t),  p = the softmax of s over the row (maximum subtracted),
        w_e = mask_e * scale (1 without a mask),  out[i] = sum_e p_e w_e h[col_e],
        dp_e = <grad[row_e], h[col_e]>,  dot_i = sum_e p_e w_e dp_e,  ds_e = p_e (w_e dp_e - dot_i),  ge_e = ds_e leaky'(t_e),
        alpha_l' = (sum of ge by row) @ h,  alpha_r' = (sum of ge by column) @ h,
        grad_out[c] = sum over the edges e into column c of p_e w_e grad[row_e]  (the transposed aggregation alone),
    and the magnitude of the terms the alpha gradients sum:  mag_e = p_e (|w_e dp_e| + |dot_i|) leaky'(t_e),
        scale_l = (sum of mag by row) @ |h|,  scale_r = (sum of mag by column) @ |h|.
    mask: [ne][heads] of 0 / 1.  Returns t, p [ne][heads], out, grad_out [n][len], alpha_l', alpha_r', scale_l, scale_r [len],
    all fp64.  A row without an edge has no t and no p; its out row is 0."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(colidx).astype(np.int64)
    rows = rows_of(rowptr)
    h = np.asarray(h, np.float64)
    g = np.asarray(grad, np.float64)
    al, ar = np.asarray(alpha_l, np.float64), np.asarray(alpha_r, np.float64)
    n, d = h.shape
    ne, dh = len(col), d // heads
    assert dh * heads == d and len(rows) == ne
    t, p = np.zeros((ne, heads)), np.zeros((ne, heads))
    out, grad_out = np.zeros((n, d)), np.zeros((n, d))
    lg, rg, scale_l, scale_r = np.zeros(d), np.zeros(d), np.zeros(d), np.zeros(d)
    for k in range(heads):
        sl = slice(k * dh, (k + 1) * dh)
        hk, gk = h[:, sl], g[:, sl]
        tk = (hk @ al[sl])[rows] + (hk @ ar[sl])[col]
        s = np.where(tk > 0, tk, eps * tk)
        M = np.full(n, -np.inf)
        np.maximum.at(M, rows, s)
        e = np.exp(s - M[rows])
        S = np.zeros(n)
        np.add.at(S, rows, e)
        pk = e / S[rows]
        w = np.ones(ne) if mask is None else np.asarray(mask, np.float64).reshape(ne, heads)[:, k] * float(scale)
        pw = pk * w
        np.add.at(out[:, sl], rows, pw[:, None] * hk[col])
        np.add.at(grad_out[:, sl], col, pw[:, None] * gk[rows])
        dp = (gk[rows] * hk[col]).sum(1)
        dot = np.zeros(n)
        np.add.at(dot, rows, pw * dp)
        slope = np.where(tk > 0, 1.0, eps)
        ge = pk * (w * dp - dot[rows]) * slope
        mag = pk * (np.abs(w * dp) + np.abs(dot[rows])) * slope
        by_row, by_col, mag_row, mag_col = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        np.add.at(by_row, rows, ge)
        np.add.at(by_col, col, ge)
        np.add.at(mag_row, rows, mag)
        np.add.at(mag_col, col, mag)
        lg[sl], rg[sl] = by_row @ hk, by_col @ hk
        scale_l[sl], scale_r[sl] = mag_row @ np.abs(hk), mag_col @ np.abs(hk)
        t[:, k], p[:, k] = tk, pk
    return t, p, out, grad_out, lg, rg, scale_l, scale_r


def alpha_ratio(got, ref, scale) -> float:
    """max_j |got_j - ref_j| / scale_j: an alpha gradient's error in units of the magnitude its sum went through"""
    got, ref, scale = (np.asarray(a, np.float64) for a in (got, ref, scale))
    assert (scale > 0).all()
    return float(np.max(np.abs(got - ref) / scale))


# ---- the graphs -----------------------------------------------------------------------------------------------------------------
N = 400
HUB = 0  # the long row of both graphs


def _with_selfloops(n, rowptr, colidx):
    key = np.unique(np.concatenate([rows_of(rowptr) * n + colidx.astype(np.int64), np.arange(n, dtype=np.int64) * (n + 1)]))
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, key // n + 1, 1)
    return np.cumsum(rp), (key % n).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def graph_a():
    """400 vertices with self loops, columns ascending in every row: row 0 has 301 edges (four chunks of 64 and one of 45),
    row 350 exactly 64, row 351 exactly 65, row 399 its self loop alone.  Returns (rowptr int64, colidx uint32)."""
    n, r64, r65, lone = N, 350, 351, N - 1
    rng = np.random.default_rng(7)
    m = n * 7 // 2
    prob = np.arange(1, n + 1, dtype=np.float64) ** -0.7
    prob /= prob.sum()
    src, dst = rng.choice(n, m, p=prob), rng.choice(n, m, p=prob)
    special = (HUB, r64, r65, lone)
    keep = ~np.isin(src, special) & ~np.isin(dst, special)  # the four special rows are built below
    src, dst = src[keep], dst[keep]
    others = np.setdiff1d(np.arange(n), special)
    extra = [(HUB, v) for v in rng.choice(others, 298, replace=False)] + [(HUB, r64), (HUB, r65)]  # 300 neighbours
    extra += [(r64, v) for v in rng.choice(others, 62, replace=False)]   # + the hub + itself = 64
    extra += [(r65, v) for v in rng.choice(others, 63, replace=False)]   # + the hub + itself = 65
    src = np.concatenate([src, [a for a, _ in extra]])
    dst = np.concatenate([dst, [b for _, b in extra]])
    rp, ci = _with_selfloops(n, *csr_from_pairs(n, src, dst))
    deg = np.diff(rp)
    assert deg[HUB] == 301 and deg[HUB] // CHUNK == 4 and deg[HUB] % CHUNK == 45
    assert deg[r64] == CHUNK and deg[r65] == CHUNK + 1 and deg[lone] == 1 and (deg >= 1).all()
    assert all((np.diff(ci[rp[i]:rp[i + 1]].astype(np.int64)) > 0).all() for i in range(n))  # ascending, duplicate-free
    assert 4.0 <= deg.mean() - 1 <= 10.0 and rp[-1] <= 4000
    return rp, ci


@functools.lru_cache(maxsize=None)
def graph_b():
    """400 vertices WITHOUT self loops: a hub row, at least 10 rows without an edge and at least 10 rows of one edge"""
    rp, ci = random_graph(N, 3, 5, power_law=True, hub_deg=200)
    deg = np.diff(rp)
    assert (deg == 0).sum() >= 10 and (deg == 1).sum() >= 10 and deg[HUB] >= 200 and rp[-1] <= 4000
    return rp, ci


def graph_of(family):
    return graph_b() if family == "benign" else graph_a()


# ---- the input families -----------------------------------------------------------------------------------------------------------
# (family, len, heads) -> seed, where the default draw misses the family's own asserts (wide: max |t| of 80.5) or takes the
# fp32 oracle itself past assert_close's default (desc: its grad_out 1.3e-4 from fp64)
_SEEDS = {("wide", 128, 16): 3, ("desc", 128, 2): 1}


@functools.lru_cache(maxsize=None)
def family(name, d, heads):
    """(rowptr, colidx, h, alpha_l, alpha_r, grad) of one family at one shape, fp32, and the family's asserts on the fp64
    scores"""
    assert name in FAMILIES and d % heads == 0
    rp, ci = graph_of(name)
    n, dh = len(rp) - 1, d // heads
    seed = _SEEDS.get((name, d, heads), 1000 * d + heads)
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    normal = lambda *shape: rng.standard_normal(shape)
    h, grad = normal(n, d), normal(n, d)
    if name in ("wide", "underflow"):
        f = (10.0 if name == "wide" else 30.0) / np.sqrt(dh)
        al, ar = normal(d) * f, normal(d) * f
    elif name in ("asc", "desc"):
        w = normal(d)
        u = np.linspace(-1.0, 1.0, n)
        h = (u if name == "asc" else u[::-1])[:, None] * w + 0.1 * h
        al, ar = 0.2 * normal(d), 50.0 * w / dh
    elif name == "uniform":
        al, ar = normal(d), np.zeros(d)
    elif name == "zero":
        al, ar = np.zeros(d), np.zeros(d)
    else:
        al, ar = 0.2 * normal(d), 0.2 * normal(d)
    h, grad, al, ar = (np.ascontiguousarray(a, np.float32) for a in (h, grad, al, ar))
    check_family(name, rp, ci, h, al, ar, heads)
    for a in (h, grad, al, ar):
        a.setflags(write=False)
    return rp, ci, h, al, ar, grad


def scores64(rp, ci, h, al, ar, heads):
    n, d = h.shape
    h3 = h.astype(np.float64).reshape(n, heads, d // heads)
    sl = (h3 * al.astype(np.float64).reshape(heads, -1)).sum(2)
    sr = (h3 * ar.astype(np.float64).reshape(heads, -1)).sum(2)
    return sl[rows_of(rp)] + sr[ci.astype(np.int64)]


def check_family(name, rp, ci, h, al, ar, heads):
    """what the family promises, on the fp64 scores of the fp32 inputs"""
    t = scores64(rp, ci, h, al, ar, heads)
    s = np.where(t > 0, t, 0.2 * t)
    hub = s[rp[HUB]:rp[HUB + 1]]
    top = np.abs(t).max()
    if name == "wide":
        assert 40 <= top <= 80, top
    elif name in ("asc", "desc"):
        assert top >= 40, top
        last = (len(hub) - 1) // CHUNK * CHUNK  # the first edge of the row's last, short chunk
        assert 0 < len(hub) - last < CHUNK
        where = hub.argmax(0)
        assert (where >= last).all() if name == "asc" else (where < CHUNK).all(), where
    elif name == "underflow":
        assert (hub.max(0) - hub.min(0)).max() > 104, hub.max(0) - hub.min(0)
    elif name == "uniform":
        assert (t == t[rp[rows_of(rp)]]).all() and top > 0  # one score per (row, head)
    elif name == "zero":
        assert (t == 0).all()
    else:
        assert top <= 12, top  # the suite's usual range


# ---- the reference and the fp32 oracle on one case, computed once ----------------------------------------------------------------
def reference(rp, ci, h, al, ar, grad, heads, mask=None, scale=1.0):
    names = ("t", "p", "out", "grad_out", "lg", "rg", "scale_l", "scale_r")
    return SimpleNamespace(**dict(zip(names, gat_ref64(rp, ci, h, al, ar, grad, heads, mask=mask, scale=scale))))


def oracle(rp, ci, h, al, ar, grad, heads):
    """the fp32 oracle's forward and backward (oracle/binding.py; it has no dropout), head by head"""
    from oracle import binding as orc

    g_o = orc.Graph(rp, ci)
    out, temp, _, p = orc.gat_aggregate_mh(g_o, h, al, ar, heads)
    grad_out, _, dp, lg, rg = orc.gat_d_aggregate_mh(g_o, h, grad, p, temp, heads)
    return SimpleNamespace(out=out, temp=temp, p=p, dp=dp, grad_out=grad_out, lg=lg, rg=rg)


@functools.lru_cache(maxsize=None)
def family_reference(name, d, heads):
    """(fp64 reference, fp32 oracle) of family(name, d, heads)"""
    ins = family(name, d, heads)
    return reference(*ins, heads), oracle(*ins, heads)
