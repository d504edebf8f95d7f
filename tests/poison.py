"""Helpers of the poison tests (tests/test_poison_cpu.py, tests/test_gpu_poison_agg.py, _dense.py, _gat.py).

The aggregation, dense-product and GAT kernels avoid branches by loading from a dummy address (row 0 of the table, a
clamped row, a neighbouring row of the operand) and multiplying by a zero weight, selecting the value away, or summing it
into a lane, row or column that is never stored.  Each is a claim that memory is read without the result depending on it;
on finite data a violation is invisible (0 * x == 0).  The method, one for all files and without a tolerance:

  * every case runs twice, `clean` on finite inputs and `poisoned` on the same inputs with a poison set overwritten (+inf;
    NaN only where no relu epilogue follows);
  * the host derives the DEPENDENT set from the operation's definition (the adjacency, the row / column index, the head of a
    column): the output entries whose defining sum contains a poisoned operand;
  * independent entries keep the clean run's bits (uint32 view); dependent entries have the class the definition gives
    (+inf where every weight on the path is positive, "not finite" where signs mix);
  * the clean run passes an fp64 check of its own;
  * outputs are pre-filled with a NaN bit pattern, 64 elements past the end included, which come back untouched; input
    tables are views into a larger allocation with NaN guard rows before and after (GUARD elements, a multiple of 64
    floats: the view keeps the alignment the dispatch looks at).

Two conditions keep a case from hiding a failure (`shares`): the independent set is at least half of the output, and the
dependent set is not empty.

This module holds what needs no GPU -- the graph, the placements, the dependent sets, the case lists -- plus the few device
helpers (they import torch when called).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from util import csr_from_pairs

NV = 613                                        # no multiple of 16
EXACT = (0, 1, 7, 8, 9, 63, 64, 65, 128, 129)   # rows of exactly this many edges (without self loops)
HUB_DEG = (150, 330)                            # heavy under spmm_heavy_threshold = 100
HEAVY = 100
GUARD = 256                                     # guard elements before and after a table: 4 x 64 floats
TAIL = 64                                       # NaN elements past the end of every output
NAN_BITS = 0x7FC0DEAD                           # the pre-fill: a quiet NaN with a payload no kernel produces
PLACEMENTS = ("row0", "last", "some", "elems")
KINDS = ("gcn", "mean", "mean_t", "edge", "edge_t")


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def graph(selfloop: bool = False) -> SimpleNamespace:
    """The poison graph: NV vertices, symmetric, sorted.  `exact[k]` is the vertex whose row has exactly k edges, `hubs` the two
    hub rows (HUB_DEG edges), vertices 0 and NV - 1 have exactly two light neighbours each; every special vertex is adjacent to
    `leaves` only, which also carry ~2 random leaf-leaf edges each.  selfloop: the same graph with (i, i) in every row (degrees
    one higher) -- for W_GCN and GAT."""
    rng = np.random.default_rng(0x9015)
    nv = NV
    exact = {k: 20 + 41 * i for i, k in enumerate(EXACT)}       # 20, 61, .., 389: spread over the 16-row strips
    hubs = (433, 517)
    special = set(exact.values()) | set(hubs) | {0, nv - 1}
    leaves = np.array([v for v in range(nv) if v not in special])
    src, dst = [], []
    want = {v: k for k, v in exact.items()}
    want.update({hubs[0]: HUB_DEG[0], hubs[1]: HUB_DEG[1], 0: 2, nv - 1: 2})
    for v, k in want.items():
        nb = rng.choice(leaves, k, replace=False)
        src += [v] * k
        dst += list(nb)
    ll = rng.choice(leaves, (600, 2))
    src += list(ll[:, 0])
    dst += list(ll[:, 1])
    rp, ci = csr_from_pairs(nv, src, dst)
    if selfloop:
        rows = np.repeat(np.arange(nv), np.diff(rp))
        key = np.unique(np.concatenate([rows * nv + ci.astype(np.int64), np.arange(nv) * (nv + 1)]))
        ci = (key % nv).astype(np.uint32)
        rp = np.concatenate([[0], np.cumsum(np.bincount(key // nv, minlength=nv))]).astype(np.int64)
    deg = np.diff(rp)
    rows = np.repeat(np.arange(nv), deg)
    _ro(rp, ci, deg, rows, leaves)
    return SimpleNamespace(nv=nv, ne=len(ci), rp=rp, ci=ci, deg=deg, rows=rows, exact=exact, hubs=hubs, leaves=leaves,
                           selfloop=selfloop, loop=1 if selfloop else 0)


def check_graph(G) -> None:
    """what the builder promises (asserted by the CPU test and before a GPU file uses the graph)"""
    lo = G.loop
    assert G.nv % 16 != 0 and np.all(np.diff(G.rp) >= 0) and G.rp[-1] == G.ne
    for k, v in G.exact.items():
        assert G.deg[v] == k + lo, (k, v, G.deg[v])
    for h, k in zip(G.hubs, HUB_DEG):
        assert G.deg[h] == k + lo and G.deg[h] > HEAVY
    light = np.ones(G.nv, bool)
    light[list(G.hubs)] = False
    assert G.deg[light].max() <= 129 + lo
    for v in (0, G.nv - 1):
        nb = [j for j in neighbours(G, v) if j != v]
        assert len(nb) == 2 and all(G.deg[j] <= HEAVY for j in nb)
    for i in range(G.nv):  # sorted, duplicate-free, symmetric
        r = G.ci[G.rp[i]:G.rp[i + 1]].astype(np.int64)
        assert np.all(np.diff(r) > 0)
    A = pattern(G)
    assert np.array_equal(A, A.T) and bool(A.diagonal().all()) == G.selfloop


def neighbours(G, v):
    return G.ci[G.rp[v]:G.rp[v + 1]].astype(np.int64)


def pattern(G) -> np.ndarray:
    """dense boolean adjacency"""
    A = np.zeros((G.nv, G.nv), bool)
    A[G.rows, G.ci.astype(np.int64)] = True
    return A


@functools.lru_cache(maxsize=None)
def some_rows(selfloop: bool = False) -> tuple:
    """about 3 % of the rows (18 leaves): the first hub is adjacent to one of them, the second hub to none"""
    G = graph(selfloop)
    a, b = (set(neighbours(G, h)) for h in G.hubs)
    only_a = sorted(a - b)
    free = sorted(set(G.leaves) - a - b)
    rows = tuple(only_a[:2] + free[3:19])
    assert len(rows) == 18 and not (set(rows) & b) and (set(rows) & a)
    return rows


@functools.lru_cache(maxsize=None)
def quiet_rows(selfloop: bool = True) -> tuple:
    """rows 0, NV - 1 and two leaves, none of them adjacent to a hub (the GAT file's NaN rows)"""
    G = graph(selfloop)
    a, b = (set(neighbours(G, h)) for h in G.hubs)
    free = sorted(set(G.leaves) - a - b)
    rows = (0, G.nv - 1, free[0], free[len(free) // 2])
    assert not (set(rows) & (a | b))
    return rows


def poison_mask(G, placement: str, d: int, nc: int | None = None) -> np.ndarray:
    """bool [nc x d]: the table entries a placement overwrites"""
    nc = G.nv if nc is None else nc
    m = np.zeros((nc, d), bool)
    if placement == "row0":
        m[0] = True
    elif placement == "last":
        m[nc - 1] = True
    elif placement == "some":
        m[list(some_rows(G.selfloop))] = True
    elif placement == "elems":
        for r in some_rows(G.selfloop)[:4] + (0,):
            m[r, 0] = m[r, d - 1] = True
    else:
        raise ValueError(placement)
    return m


def dependent(G, pmask: np.ndarray) -> np.ndarray:
    """bool [nv x d]: out[i, c] = sum over the edges (i, j) of w * x[j, c] contains a poisoned x[j, c].  The same for all five
    weight kinds: the graph is symmetric and every weight is positive, W_EDGE_T only takes the weight from the reverse edge."""
    dep = np.zeros((G.nv, pmask.shape[1]), np.int64)
    np.add.at(dep, G.rows, pmask[G.ci.astype(np.int64)].astype(np.int64))
    return dep > 0


def dependent_edge_w(G, kind: str, rows, heads_hit, heads: int, d: int) -> np.ndarray:
    """bool [nv x d] under EDGE-WEIGHT poison: ew[e, h] = +inf on every edge e of the rows `rows`, for h in heads_hit.
    W_EDGE: those rows; W_EDGE_T (out[i] takes ew of the reverse edge (j, i), which lies in row j): the rows adjacent to them.
    Head h's columns only."""
    dh = d // heads
    hit = np.zeros(G.nv, bool)
    if kind == "edge":
        hit[[r for r in rows if G.deg[r] > 0]] = True
    else:
        for r in rows:
            hit[neighbours(G, r)] = True
    dep = np.zeros((G.nv, d), bool)
    for h in heads_hit:
        dep[np.ix_(hit, np.arange(h * dh, (h + 1) * dh))] = True
    return dep


def reverse_edges(G) -> np.ndarray:
    """rev[e] = the index of edge (j, i) for e = (i, j)"""
    key = G.rows * G.nv + G.ci.astype(np.int64)
    back = G.ci.astype(np.int64) * G.nv + G.rows
    rev = np.searchsorted(key, back)
    assert np.array_equal(key[rev], back)
    return rev


def edge_weights(G, heads: int = 1, seed: int = 3) -> np.ndarray:
    """positive fp32 weights [ne] or [ne x heads] of the size attention has: (0.5 + u) / deg(row)"""
    u = np.random.default_rng(seed).random((G.ne, heads)).astype(np.float32)
    w = ((np.float32(0.5) + u) / np.maximum(G.deg[G.rows], 1)[:, None].astype(np.float32)).astype(np.float32)
    return w[:, 0].copy() if heads == 1 else w


def weights64(G, kind: str, ew=None) -> np.ndarray:
    """the per-edge weights of a kind in fp64, [ne] or [ne x heads], as the library defines them: deg^-1/2 on both ends,
    1 / deg(row), 1 / deg(column), the edge weights, the reverse edges' weights"""
    deg = G.deg.astype(np.float64)
    inv = np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)
    r, c = G.rows, G.ci.astype(np.int64)
    if kind == "gcn":
        return np.sqrt(inv[r]) * np.sqrt(inv[c])
    if kind == "mean":
        return inv[r]
    if kind == "mean_t":
        return inv[c]
    if kind == "edge":
        return np.asarray(ew, np.float64)
    if kind == "edge_t":
        return np.asarray(ew, np.float64)[reverse_edges(G)]
    raise ValueError(kind)


def aggregate64(G, kind: str, x, ew=None, heads: int = 1) -> np.ndarray:
    """fp64 aggregation from the definition (inf and NaN travel as IEEE says)"""
    x = np.asarray(x, np.float64)
    w = weights64(G, kind, ew)
    d = x.shape[1]
    if w.ndim == 2:
        w = np.repeat(w, d // heads, axis=1)
    else:
        w = w[:, None]
    out = np.zeros((G.nv, d))
    live = np.nonzero(G.deg > 0)[0]
    with np.errstate(invalid="ignore"):
        out[live] = np.add.reduceat(w * x[G.ci.astype(np.int64)], G.rp[:-1][live], axis=0)  # (rows are contiguous in the CSR)
    return out


def features(n: int, d: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def shares(dep: np.ndarray, what: str = "") -> None:
    """the two conditions that keep a case honest"""
    dep = np.asarray(dep, bool)
    assert dep.any(), f"{what}: no dependent entry"
    assert 2 * int(dep.sum()) <= dep.size, f"{what}: {int(dep.sum())} of {dep.size} entries dependent, more than half"


def bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64 if a.dtype.itemsize == 8 else np.uint16)


def compare(clean, poisoned, dep, cls: str, what: str = "") -> None:
    """assertions 1 and 2: independent entries keep their bits; dependent ones are `cls`: "+inf", "nonfinite",
    "+inf|0" (a relu after mixed signs: !(v > 0) -> 0), or None (recorded elsewhere, not asserted)"""
    clean, poisoned, dep = np.asarray(clean), np.asarray(poisoned), np.asarray(dep, bool)
    assert clean.shape == poisoned.shape == dep.shape, (what, clean.shape, poisoned.shape, dep.shape)
    assert np.isfinite(clean).all(), f"{what}: the clean run is not finite"
    diff = (bits(clean) != bits(poisoned)) & ~dep
    assert not diff.any(), (f"{what}: {int(diff.sum())} independent entries changed with the poison, first at "
                            f"{tuple(int(v) for v in np.argwhere(diff)[0])}: {clean[diff][0]!r} -> {poisoned[diff][0]!r}")
    v = poisoned[dep]
    if cls == "+inf":
        bad = ~np.isposinf(v)
    elif cls == "nonfinite":
        bad = np.isfinite(v)
    elif cls == "+inf|0":
        bad = ~(np.isposinf(v) | (v == 0))
    else:
        assert cls is None, cls
        return
    assert not bad.any(), f"{what}: {int(bad.sum())} of {v.size} dependent entries are not {cls}, first {v[bad][0]!r}"


# ---- the aggregation cases ----------------------------------------------------------------------------------------------------------
SPMM_DIMS = (16, 47, 64, 128, 256, 300)   # the sub-wave kernel, the re-strided copy, one, two and more column tiles
MH_SHAPES = ((4, 64), (8, 64), (4, 256), (8, 256))  # (heads, d) of the edge-weight poison
GEMM_SHAPES = ((128, 128), (100, 128), (64, 48), (256, 128))
ROWS2_POISON = (0, 7, NV - 1)


def ew_rows(G) -> tuple:
    """the three rows whose edge weights are poisoned: a light row, the row of 65 edges, the first hub"""
    return (int(some_rows(G.selfloop)[0]), G.exact[65], G.hubs[0])


def ew_heads(heads: int) -> tuple:
    return (1, heads - 1)


def n_first(G) -> int:
    """a table split inside the graph: both rows either side of it are leaves with edges"""
    leaf = np.zeros(G.nv, bool)
    leaf[G.leaves] = True
    ok = leaf & (G.deg > G.loop)
    v = 300
    while not (ok[v - 1] and ok[v]):
        v += 1
    return v


def split_mask(G, placement: str, d: int) -> np.ndarray:
    """the two-table placements: row 0 of the second table, the last row of the first, both"""
    nf = n_first(G)
    m = np.zeros((G.nv, d), bool)
    m[{"x2row0": [nf], "x1last": [nf - 1], "both": [nf - 1, nf]}[placement]] = True
    return m


def agg_cases():
    """(what, dependent mask) of every aggregation case of tests/test_gpu_poison_agg.py: the CPU test holds each to `shares`"""
    for loop in (False, True):
        G = graph(loop)
        for d in SPMM_DIMS:
            for pl in PLACEMENTS:
                yield f"spmm loop {loop} d {d} {pl}", dependent(G, poison_mask(G, pl, d))
        for pl in ("x2row0", "x1last", "both"):
            yield f"2t loop {loop} {pl}", dependent(G, split_mask(G, pl, 64))
        for heads, d in MH_SHAPES:
            for kind in ("edge", "edge_t"):
                yield f"ew loop {loop} {kind} {heads} {d}", dependent_edge_w(G, kind, ew_rows(G), ew_heads(heads), heads, d)
        for len_in, len_out in GEMM_SHAPES + ((256, 256),):
            for pl in PLACEMENTS:
                dep = dependent(G, poison_mask(G, pl, len_in))
                yield f"gemm loop {loop} {len_in} {len_out} {pl}", np.repeat(dep.any(1)[:, None], len_out, 1)
        r2 = np.zeros((G.nv, 8), bool)
        r2[list(ROWS2_POISON)] = True
        yield f"rows2 loop {loop}", r2


# ---- dense products: the forms, their shapes and their dependent sets -------------------------------------------------------------
# (form, tA, tB, M, N, K, sgemm_variant).  The variant is what sends the shape to the form named (0: the dispatch's own rule).
DENSE_FORMS = [
    ("tiled nn", 0, 0, 33, 65, 129, 0), ("tiled nt", 0, 1, 33, 65, 129, 0), ("tiled tn", 1, 0, 33, 65, 129, 0),
    ("tiled nn", 0, 0, 257, 33, 31, 0), ("tiled nt", 0, 1, 257, 33, 31, 0), ("tiled tn", 1, 0, 257, 33, 31, 0),
    ("split-K tn", 1, 0, 128, 128, 4097, 0),
    ("register tn", 1, 0, 128, 128, 32769, 0), ("register tn", 1, 0, 100, 47, 32769, 0),
    ("register tn odd N", 1, 0, 100, 67, 32769, 0),
    ("register tn teams", 1, 0, 256, 256, 32769, 0), ("register tn narrow B", 1, 0, 128, 33, 32769, 0),
    ("LDS ring tn", 1, 0, 256, 256, 32769, 35),
    ("streaming nn", 0, 0, 65, 128, 100, 41), ("streaming nt", 0, 1, 65, 128, 100, 41),
    ("streaming nn", 0, 0, 65, 200, 256, 41), ("streaming nt", 0, 1, 65, 96, 256, 41),
    ("row-stream nn", 0, 0, 65537, 47, 128, 0), ("row-stream nt", 0, 1, 65537, 128, 47, 0),
    ("row-stream nn ragged K", 0, 0, 65537, 128, 47, 0), ("row-stream nt short K", 0, 1, 65537, 64, 40, 0),
    ("skinny tn", 1, 0, 128, 47, 65537, 0),
    ("wide tn", 1, 0, 100, 128, 65537, 0),
]


def dense_dependent(M: int, N: int, side: str) -> np.ndarray:
    """odd rows of the M-side operand (rows of A; columns of A for TN) -> odd rows of C; odd columns of the N-side operand
    (columns of B; rows of B for NT) -> odd columns of C"""
    dep = np.zeros((M, N), bool)
    if side == "M":
        dep[1::2] = True
    else:
        dep[:, 1::2] = True
    return dep


def dense_poison(A: np.ndarray, B: np.ndarray, tA: int, tB: int, side: str):
    """(A, B) with every odd row / column of the named side's operand at +inf"""
    A, B = A.copy(), B.copy()
    if side == "M":
        if tA:
            A[:, 1::2] = np.inf
        else:
            A[1::2] = np.inf
    elif tB:
        B[1::2] = np.inf
    else:
        B[:, 1::2] = np.inf
    return A, B


# ---- device helpers -----------------------------------------------------------------------------------------------------------------
def nan_fill(t):
    """fill a float32 / bfloat16 device tensor with the NaN pre-fill pattern"""
    import torch

    if t.dtype == torch.float32:
        t.view(torch.int32).fill_(NAN_BITS)
    else:
        t.view(torch.int16).fill_(0x7FC1)
    return t


def table(a, dtype=None):
    """the numpy array `a` as a device tensor that is a view into a larger allocation: GUARD NaN elements before and after"""
    import torch

    src = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        src = src.to(dtype)
    buf = nan_fill(torch.empty(src.numel() + 2 * GUARD, dtype=src.dtype, device="cuda"))
    view = buf[GUARD:GUARD + src.numel()].view(src.shape)
    view.copy_(src)
    assert (view.data_ptr() - buf.data_ptr()) % 256 == 0
    return view


class Out:
    """an output [shape] pre-filled with NaN bits, TAIL elements past its end included"""

    def __init__(self, *shape, fill=None):
        import torch

        n = int(np.prod(shape))
        self.buf = nan_fill(torch.empty(n + TAIL, device="cuda"))
        self.t = self.buf[:n].view(*shape)
        if fill is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill)))

    def host(self, what: str = "", written: bool = True) -> np.ndarray:
        """the output on the host; the tail must be untouched, and (written) nothing of the pre-fill may survive"""
        a = self.buf.cpu().numpy()
        n = a.size - TAIL
        assert (bits(a[n:]) == NAN_BITS).all(), f"{what}: the {TAIL} elements past the end were written"
        out = a[:n].reshape(tuple(self.t.shape))
        if written:
            assert not (bits(out) == NAN_BITS).any(), f"{what}: left unwritten"
        return out
