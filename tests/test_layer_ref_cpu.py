"""The fp64 layer references (tests/layer_ref64.py) and the operands of the exact layer tests, without a GPU:
  * the 2^24 bounds hold, from the data, over the case lists tests/test_gpu_layers_exact.py iterates;
  * layer_ref64 agrees with torch fp64 autograd of the forward definition (GCN, SAGE: dW, dW_self, grad_out);
  * on the integer data the oracle's fp32 GCNLayer / SAGELayer equal layer_ref64 BIT FOR BIT at both levels, with and without
    the activation and under a seeded feature-dropout mask (the oracle runs on D(X), its grad_out gets the mask and the scale):
    the in-place d_relu on grad_in and the level-0 rule are the reference's;
  * the oracle's GAT layer on D(X) lies within 1e-4 (util.ELEM_RTOL, both metrics, test_gpu_gat_extremes.close) of
    gat_layer_ref64 on the cases of tests/test_gpu_gat_layers64.py, so the rule those cells are judged by -- rtol = max(1e-4,
    twice the oracle's distance) -- stays at 1e-4 or close to it;
  * a one-entry corruption of each output is noticed by the comparison helpers;
  * a score moved to within 1e-9 of 0 is listed as undecided, and its listed change is the difference of the two references."""
import numpy as np
import pytest
import torch

import exact as E
import gat_ref64 as R
import layer_ref64 as LR
import poison as P
from oracle import binding as orc
from test_gpu_gat_extremes import alpha_close, close

SHAPE_IDS = [f"{a}x{b}" for a, b in LR.SHAPES]


def test_the_graphs():
    for kind in LR.KINDS:
        G = LR.graph_of(kind)
        E.check_regular(G)
        assert G.nv == 1538 and G.selfloop == (kind == "gcn")
        w = np.concatenate([P.weights64(G, k) for k in (("gcn",) if kind == "gcn" else ("mean", "mean_t"))])
        assert np.array_equal(np.log2(w), np.rint(np.log2(w))) and w.min() == E.UNIT  # powers of two, the smallest 2^-10
    rp, ci = LR.gat_graph()
    deg = np.diff(rp)
    assert len(deg) == LR.GAT_N and deg[R.HUB] > 4 * R.CHUNK and all(i in ci[rp[i]:rp[i + 1]] for i in range(len(deg)))
    back = np.sort(ci.astype(np.int64) * LR.GAT_N + R.rows_of(rp))
    assert np.array_equal(back, R.rows_of(rp) * LR.GAT_N + ci.astype(np.int64))  # symmetric


def test_bounds_hold_over_the_case_lists():
    """layer_operands asserts them; the largest per kind is printed (LEDGER 27 has the figures)"""
    assert LR.scale_of(LR.RATE) == 2.0 and LR.scale_of(0.0) == 1.0
    assert set(LR.RELATION_SHAPES) <= set(LR.SHAPES) and len(LR.CELLS) == 2 * 64
    for kind in LR.KINDS:
        worst = {}
        for _, din, dout, _, _, drop in (c for c in LR.CELLS if c[0] == kind):
            ops = LR.layer_operands(kind, din, dout, drop)
            assert ops.top < E.LIMIT and ops.grange == 3, (kind, din, dout, drop, ops.grange)
            assert all(np.abs(a).max() <= 3 and np.array_equal(a, np.rint(a)) for a in (ops.x, ops.g, ops.g2, ops.W, ops.W_self))
            for k, v in ops.tops.items():
                if v > worst.get(k, (0,))[0]:
                    worst[k] = (v, din, dout, drop)
            # the bf16 routes round a table to at most 1 + 2^-8 of its magnitude
            assert ops.top * (1 + 2.0 ** -8) < E.LIMIT
        print(kind, {k: f"{v[0]:.0f} at {v[1]} -> {v[2]} drop {v[3]}" for k, v in worst.items()})


def dense_adj(G, kind):
    A = np.zeros((G.nv, G.nv))
    A[G.rows, G.ci.astype(np.int64)] = P.weights64(G, kind)
    return torch.from_numpy(A)


@pytest.fixture(scope="module")
def adj():
    return {kind: dense_adj(LR.graph_of(kind), "gcn" if kind == "gcn" else "mean") for kind in LR.KINDS}


@pytest.mark.parametrize("din,dout", LR.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", LR.KINDS)
def test_reference_agrees_with_autograd(adj, kind, din, dout):
    """the forward definition in torch fp64, differentiated by autograd: the sums are exact in fp64 in any order, so equality"""
    G, A = LR.graph_of(kind), adj[kind]
    for drop in (0.0, LR.RATE):
        ops = LR.layer_operands(kind, din, dout, drop)
        mask = LR.seeded_mask((G.nv, din), 5) if drop else None
        for act in (False, True):
            ref = LR.layer_ref64(kind, G, ops, ops.g, act, 1, mask, ops.scale)
            x = torch.from_numpy(ops.x.astype(np.float64)).requires_grad_()
            W = torch.from_numpy(ops.W.astype(np.float64)).requires_grad_()
            Ws = torch.from_numpy(ops.W_self.astype(np.float64)).requires_grad_()
            dx = x if mask is None else x * torch.from_numpy(mask.astype(np.float64)) * ops.scale
            pre = A @ dx @ W + (dx @ Ws if kind == "sage" else 0.0)
            out = torch.relu(pre) if act else pre
            (out * torch.from_numpy(ops.g.astype(np.float64))).sum().backward()
            what = f"{kind} {din} -> {dout} drop {drop} act {act}"
            assert np.array_equal(out.detach().numpy(), ref.out), what
            assert np.array_equal(W.grad.numpy(), ref.dW), what
            assert np.array_equal(x.grad.numpy(), ref.grad_out), what
            if kind == "sage":
                assert np.array_equal(Ws.grad.numpy(), ref.dW_self), what
            for a in (ref.out, ref.dW, ref.grad_out, ref.ax):
                E.assert_dyadic(a)


@pytest.mark.parametrize("din,dout", LR.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", LR.KINDS)
def test_oracle_layers_equal_the_reference_bit_for_bit(kind, din, dout):
    G = LR.graph_of(kind)
    g_o = orc.Graph(G.rp, G.ci)
    for drop in (0.0, LR.RATE):
        ops = LR.layer_operands(kind, din, dout, drop)
        mask = LR.seeded_mask((G.nv, din), 7) if drop else None
        x32 = LR.dropped(ops.x, mask, ops.scale).astype(np.float32)  # D(X): integers in [-6, 6]
        for act in (False, True):
            ref = LR.layer_ref64(kind, G, ops, ops.g, act, 1, mask, ops.scale)
            for level in (0, 1):
                what = f"{kind} {din} -> {dout} drop {drop} act {act} level {level}"
                if kind == "gcn":
                    lo = orc.GCNLayer(level, g_o, din, dout, act, W=ops.W)
                else:
                    lo = orc.SAGELayer(level, g_o, din, dout, act, W_neigh=ops.W, W_self=ops.W_self)
                LR.assert_same(lo.forward(x32), ref.out, what + " out")
                gin = np.array(ops.g)
                go = lo.backward(gin)
                LR.assert_same(gin, ref.gmask, what + " grad_in after the backward")  # d_relu ran in place
                LR.assert_same(lo.W_grad if kind == "gcn" else lo.W_neigh_grad, ref.dW, what + " dW")
                if kind == "sage":
                    LR.assert_same(lo.W_self_grad, ref.dW_self, what + " dW_self")
                if level == 0:
                    assert go is None
                else:
                    go64 = go.astype(np.float64)
                    LR.assert_same(LR.dropped(go64, mask, ops.scale).astype(np.float32), ref.grad_out, what + " grad_out")


def test_level_0_reference_has_no_grad_out():
    for kind in LR.KINDS:
        ops = LR.layer_operands(kind, 47, 128, 0.0)
        a, b = (LR.layer_ref64(kind, LR.graph_of(kind), ops, ops.g, True, level) for level in (0, 1))
        assert a.grad_out is None and b.grad_out is not None and np.array_equal(a.dW, b.dW) and np.array_equal(a.out, b.out)


def test_rounded_tables_change_only_what_depends_on_them():
    """round_xw / round_gwt (the bf16 routes): the rounded reference is still exact in fp32 and differs from the plain one"""
    for kind in LR.KINDS:
        G = LR.graph_of(kind)
        # (on these data the rounding is nearly the identity: D(X) W holds even integers of a few hundred under dropout, G' W^T
        # stays below 256 at 128 columns -- so the hook is also tried with a coarser rounding, which must show)
        coarse = lambda a: np.rint(a / 16) * 16  # noqa: E731
        ops = LR.layer_operands(kind, 300, 16, LR.RATE)
        mask = LR.seeded_mask((G.nv, 300), 9)
        plain = LR.layer_ref64(kind, G, ops, ops.g, True, 1, mask, ops.scale)
        rnd = LR.layer_ref64(kind, G, ops, ops.g, True, 1, mask, ops.scale, round_xw=LR.bf16_round)
        E.assert_dyadic(rnd.out)
        rnd = LR.layer_ref64(kind, G, ops, ops.g, True, 1, mask, ops.scale, round_xw=coarse)
        assert not np.array_equal(plain.out, rnd.out) and np.array_equal(plain.ax, rnd.ax)
        ops = LR.layer_operands(kind, 100, 128, 0.0)
        plain = LR.layer_ref64(kind, G, ops, ops.g, True, 1)
        rnd = LR.layer_ref64(kind, G, ops, ops.g, True, 1, round_gwt=LR.bf16_round)
        assert np.array_equal(plain.out, rnd.out) and np.array_equal(plain.dW, rnd.dW)
        E.assert_dyadic(rnd.grad_out)
        rnd = LR.layer_ref64(kind, G, ops, ops.g, True, 1, round_gwt=coarse)
        assert not np.array_equal(plain.grad_out, rnd.grad_out) and np.array_equal(plain.dW, rnd.dW)
    v = np.array([257.0, 259.0, 3.0, -1027.0, 5400.0])
    assert np.array_equal(LR.bf16_round(v), [256.0, 260.0, 3.0, -1024.0, 5408.0])  # ties to even


# ---- GAT ----------------------------------------------------------------------------------------------------------------------------
def gat_case(din, dout, heads, act, level, drop):
    rp, ci = LR.gat_graph()
    ops = LR.gat_operands(din, dout, heads)
    mask = LR.seeded_mask((LR.GAT_N, din), 11) if drop else None
    scale = LR.scale_of(drop)
    ref = LR.gat_layer_ref64(rp, ci, ops.x, ops.W, ops.al, ops.ar, ops.g, heads, act, level, mask, scale)
    x32 = LR.dropped(ops.x, mask, scale).astype(np.float32)  # (x * 2 and x * 0 are exact in fp32)
    return rp, ci, ops, mask, scale, ref, x32


@pytest.mark.parametrize("din,dout", LR.GAT_SHAPES, ids=[f"{a}x{b}" for a, b in LR.GAT_SHAPES])
@pytest.mark.parametrize("heads", [1, 8])
def test_oracle_gat_layer_within_the_rule(din, dout, heads):
    worst, undecided = {}, 0
    for _, _, _, act, level, drop in (c for c in LR.GAT_CELLS if c[:3] == (din, dout, heads)):
        rp, ci, ops, mask, scale, ref, x32 = gat_case(din, dout, heads, act, level, drop)
        what = f"oracle GAT {din} -> {dout} heads {heads} act {act} level {level} drop {drop}"
        print(what)
        out32 = ref.out.astype(np.float32)  # the backward runs on the reference's output: the same relu mask (oracle_gat_layer)
        o = LR.oracle_gat_layer(rp, ci, x32, ops.W, ops.al, ops.ar, ops.g, heads, act, level, mask_out=out32)
        flips = (o.out > 0) != (ref.out > 0)
        assert np.abs(ref.pre[flips]).max(initial=0.0) <= 1e-6 * np.abs(ref.pre).max(), what  # only where the output is 0 to fp32
        if heads == 1:  # the oracle's own layer composition: the same bits as its operators composed here
            lo = orc.GATLayer(level, orc.Graph(rp, ci), din, dout, act, W=ops.W, alpha_l=ops.al, alpha_r=ops.ar, fast=True)
            assert np.array_equal(lo.forward(x32), o.out), what
            lo.feat_out = out32
            go = lo.backward(np.array(ops.g))
            assert np.array_equal(lo.W_grad, o.dW) and np.array_equal(lo.alpha_lgrad, o.lg) and np.array_equal(lo.alpha_rgrad, o.rg), what
            assert go is None if level == 0 else np.array_equal(go, o.grad_out), what
        d = LR.gat_distances(o, ref, mask, scale)
        for k, v in d.items():
            worst[k] = max(worst.get(k, 0.0), v)
        # o = 0: the rule's floor of 1e-4 alone
        close(o.out, ref.out, 0.0, what + " out", long_rows=[R.HUB])
        close(o.dW, ref.dW, 0.0, what + " dW", long_rows=range(din))
        if level > 0:
            close(LR.dropped(o.grad_out, mask, scale), ref.grad_out, 0.0, what + " grad_out", long_rows=[R.HUB])
        near = LR.nearest_alpha_reference(ref, o.lg, o.rg)
        undecided += near.undecided
        alpha_close(o.lg, o.rg, near, 0.0, what)
    print(f"{undecided} undecided slopes")
    print(f"oracle GAT {din} -> {dout} heads {heads}: worst distances", {k: f"{v:.2e}" for k, v in worst.items()})


# ---- the comparison helpers notice one entry ------------------------------------------------------------------------------------------
def test_one_corrupted_entry_is_noticed():
    for kind in LR.KINDS:
        G = LR.graph_of(kind)
        ops = LR.layer_operands(kind, 64, 64, LR.RATE)
        mask = LR.seeded_mask((G.nv, 64), 13)
        ref = LR.layer_ref64(kind, G, ops, ops.g, True, 1, mask, ops.scale)
        names = ("out", "gmask", "dW", "grad_out") + (("dW_self",) if kind == "sage" else ())
        rng = np.random.default_rng(17)
        for name in names:
            want = getattr(ref, name)
            good = want.astype(np.float32)
            assert LR.mismatch(good, want, name) is None and LR.mismatch(torch.from_numpy(good), want, name) is None
            at = tuple(int(rng.integers(n)) for n in good.shape)
            for wrong in (np.nextafter(good[at], np.float32(np.inf)), np.float32(np.nan), good[at] + np.float32(E.UNIT)):
                bad = good.copy()
                bad[at] = wrong
                msg = LR.mismatch(bad, want, name)
                assert msg is not None and str(at) in msg, (kind, name, at, msg)
            with pytest.raises(AssertionError):
                LR.assert_same(bad, want, name)
        assert LR.mismatch(ref.out.astype(np.float32)[:-1], ref.out, "shape") is not None
        with pytest.raises(AssertionError):  # a reference that fp32 does not hold is refused, not rounded
            LR.mismatch(ref.out.astype(np.float32), ref.out + E.UNIT / 2, "not dyadic")


def test_one_corrupted_entry_is_noticed_by_the_gat_rule():
    rp, ci, ops, mask, scale, ref, x32 = gat_case(64, 64, 8, True, 1, LR.RATE)
    o = LR.oracle_gat_layer(rp, ci, x32, ops.W, ops.al, ops.ar, ops.g, 8, True, 1, mask_out=ref.out.astype(np.float32))
    d = LR.gat_distances(o, ref, mask, scale)
    rng = np.random.default_rng(19)
    for name, long_rows in (("out", [R.HUB]), ("dW", range(64)), ("grad_out", [R.HUB])):
        want = getattr(ref, name)
        got = getattr(o, name).astype(np.float64)
        if name == "grad_out":
            got = LR.dropped(got, mask, scale)
        close(got, want, d[name], name, long_rows=long_rows)
        at = tuple(int(rng.integers(n)) for n in want.shape)
        got[at] += 1e-3 * np.abs(want).max()
        with pytest.raises(AssertionError):
            close(got, want, d[name], name, long_rows=long_rows)
    lg = o.lg.astype(np.float64)
    alpha_close(lg, o.rg, ref, d["alpha"], "alpha")
    lg[3] += 1e-4 * ref.scale_l[3]
    with pytest.raises(AssertionError):
        alpha_close(lg, o.rg, ref, d["alpha"], "alpha")


def test_an_undecided_slope_is_found_and_its_other_reference_is_exact():
    """a score moved to within fp32's error of 0 is listed by undecided_slopes, and the listed change of the alpha gradients is the
    difference between the references on either side of 0"""
    rp, ci = LR.gat_graph()
    ops = LR.gat_operands(64, 64, 8)
    base = LR.gat_layer_ref64(rp, ci, ops.x, ops.W, ops.al, ops.ar, ops.g, 8, False, 1)
    e, k = int(np.abs(base.t[:, 3]).argmin()), 3   # head 3's score nearest 0: shift alpha_r's head-3 block until it is +-1e-9
    rows, col = R.rows_of(rp), ci.astype(np.int64)
    h = base.h[:, 24:32]
    refs = {}
    for side in (1.0, -1.0):
        ar = ops.ar.astype(np.float64)
        ar[24:32] += (side * 1e-9 - base.t[e, k]) * h[col[e]] / (h[col[e]] @ h[col[e]])
        refs[side] = LR.gat_layer_ref64(rp, ci, ops.x, ops.W, ops.al, ar, ops.g, 8, False, 1)
        assert abs(refs[side].t[e, k] - side * 1e-9) < 1e-12 and len(refs[side].undecided) >= 1
    up, down = refs[1.0], refs[-1.0]
    near = LR.nearest_alpha_reference(up, down.lg, down.rg)  # the reference below 0 is the one above with that slope flipped
    assert near.flipped >= 1
    assert max(R.alpha_ratio(down.lg, near.lg, up.scale_l), R.alpha_ratio(down.rg, near.rg, up.scale_r)) < 1e-6 * 2.0 ** -24 * 1e3
    assert max(R.alpha_ratio(down.lg, up.lg, up.scale_l), R.alpha_ratio(down.rg, up.rg, up.scale_r)) > 2.0 ** -24  # ... and it matters
