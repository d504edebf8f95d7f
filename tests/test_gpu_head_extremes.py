"""GPU suite, the kernels of csrc/elementwise.hip where the rest of the suite never takes them (tests/head_ref64.py has the
references and the inputs): logits offset by +-3e4, spread over 80 and past 110 below the row maximum (the clamp loss), tied and
all-equal logits, a single logit at 1e4; sigmoid logits of scale 100 and 1e4 and of exactly 0.0, -0.0 and +-88.8; class counts
around the 64 lanes of a wave; a range of 193 rows from row 5 (a partial last block); masks that are absent, sparse, empty, full
and hold the byte 2; metrics over integer losses (exact in any order), tied, -inf and NaN predictions, predictions of exactly 0.5,
label bytes of 2, more rows than the 1024-block cap covers at once; l2norm at row lengths around 64 and 128 and at 1000, on rows
of 0, 1e-8 and 1e15; Adam one step at a time at lengths that are no multiple of 256 and above the grid cap, at steps 1, 10 and
5000, on gradients of 0, 1e-6..1e-4 and 1e18; relu on NaN, +-0, +-inf and subnormals, aligned, from 4-byte-aligned pointers and in
place; bias_add / colsum / fill / scale at both ends of their loops; sgemm with K, M or N of 0.

What is held to what:
  * bits, where the operation is exact: counts, ratios of counts, integer sums, relu, bias_add, fill, scale, the clamp loss, the
    _dev forms against the host forms, and everything an operation does not define -- every output is pre-filled with a NaN bit
    pattern (CANARY), 64 elements past its end included, rows outside the range and outside the mask carry NaN logits;
  * a derived bound, where the code fixes the length of a summation chain: masked_avg_loss on real losses and colsum on Gaussian
    data (the derivations stand at the two tests);
  * GPU_FACTOR = 4 times the fp32 oracle's own distance from fp64 per operation and family (head_ref64.ORACLE_DIST, asserted by
    tests/test_head_extremes_cpu.py) for probabilities, losses, gradients, l2norm and Adam, in the metrics of head_ref64
    (probabilities scaled by 1 + |x - max|, losses by 1 + |loss|, Adam's m and update by what they were summed from); the
    forward results also pass util.assert_close's pair (1e-4 / 1e-6).
Each test prints its worst figures (pytest -s); LEDGER 22 has them."""
import numpy as np
import pytest
import torch

import head_ref64 as R
from graphaibench_amd import capi
from util import assert_close

pytestmark = pytest.mark.gpu

BEGIN, END, N = R.HEAD_BEGIN, R.HEAD_END, R.HEAD_N
CANARY = 0x7FC0BEEF  # a quiet NaN with a payload: read by mistake it spreads, overwritten it shows
PAD = 64
SEEN = {}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the families' arrays are read-only)


def canary(n, init=None):
    """n + PAD floats of CANARY on the device, the first n set to `init` where given"""
    t = torch.full((n + PAD,), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)
    if init is not None:
        t[:n] = dev(np.ascontiguousarray(init, np.float32).ravel())
    return t


def bits(t):
    if isinstance(t, torch.Tensor):
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return np.ascontiguousarray(t, np.float32).view(np.uint32)


def f32(b):
    return b.view(np.float32)


def untouched(b, what):
    assert (b == CANARY).all(), f"{what}: {int((b != CANARY).sum())} elements written that the operation does not define"


def held(op, family, value, what):
    SEEN[(op, family)] = max(SEEN.get((op, family), 0.0), value)
    assert value <= R.bound(op, family), f"{what}: {op} {value:.3e}, bound {R.bound(op, family):.3e} (oracle {R.ORACLE_DIST[(op, family)]:.3e})"


def report(head, ops, families):
    """the worst figures so far (over the cases of this session up to `head`)"""
    for op in ops:
        print(f"  {head} {op}: " + "  ".join(f"{f} {SEEN.get((op, f), 0.0):.2e}" for f in families))


def nan_outside(x, rows):
    """a copy of x with NaN in every row the operation must not read"""
    y = np.full_like(x, np.nan)
    y[rows] = x[rows]
    return y


# ---- the loss heads ----------------------------------------------------------------------------------------------------------
def run_softmax(ctx, x, lab, mk, fam, what):
    Cn = x.shape[1]
    ref = R.softmax_xent(x, lab, BEGIN, END, mk)
    other = np.setdiff1d(np.arange(N), ref.rows)
    probs, loss, diff = canary(N * Cn), canary(N), canary(N * Cn)
    labd, mkd = dev(lab), (dev(mk) if mk is not None else None)
    ctx.softmax_xent(dev(nan_outside(x, ref.rows)), labd, loss[:N], probs[:N * Cn].view(N, Cn), BEGIN, END, masks=mkd)
    pb, lb = bits(probs), bits(loss)
    untouched(pb[N * Cn:], what + " probabilities, past the end")
    untouched(lb[N:], what + " loss, past the end")
    pb = pb[:N * Cn].reshape(N, Cn)
    untouched(pb[other], what + " probabilities")
    untouched(lb[other], what + " loss")
    p, l = f32(pb)[ref.rows], f32(lb[:N])[ref.rows]
    assert np.array_equal(bits(l[ref.clamp]), bits(np.full(int(ref.clamp.sum()), R.CLAMP32))), what + ": the clamp loss"
    held("softmax_p", fam, R.prob_err(p, ref.p, ref.xm), what)
    held("softmax_loss", fam, R.loss_err(l, ref.loss), what)
    assert_close(p, ref.p, what + " probabilities")
    assert_close(l, ref.loss, what + " loss")
    ctx.d_softmax_xent(probs[:N * Cn].view(N, Cn), labd, diff[:N * Cn].view(N, Cn), BEGIN, END, masks=mkd)
    db = bits(diff)
    untouched(db[N * Cn:], what + " gradient, past the end")
    db = db[:N * Cn].reshape(N, Cn)
    untouched(db[other], what + " gradient")
    dref = R.d_softmax_xent(f32(pb), lab, BEGIN, END, mk)
    held("d_softmax", fam, R.rel_elem_err(f32(db)[dref.rows], dref.diff, tiny=R.P_NORMAL), what)
    return ref


@pytest.mark.parametrize("Cn", R.SOFTMAX_CLS)
def test_softmax_head(ctx, Cn):
    for fam in R.SOFTMAX_FAMILIES:
        x, lab = R.softmax_family(fam, Cn)
        for mkind in R.MASKS:
            ref = run_softmax(ctx, x, lab, R.mask_of(mkind), fam, f"softmax {fam} C={Cn} mask {mkind}")
            assert len(ref.rows) == {"none": 193, "third": 65, "zeros": 0, "ones": 193}.get(mkind, len(ref.rows))
            if fam == "clamp" and Cn > 1:
                assert ref.clamp.all()
    report(f"C={Cn}", ("softmax_p", "softmax_loss", "d_softmax"), R.SOFTMAX_FAMILIES)


def test_softmax_label_that_is_no_class(ctx):
    """a label byte >= num_cls (200 at 7 classes): the clamp loss, the row's probabilities as ever, nothing else touched"""
    x, lab = R.softmax_family("benign", 7)
    lab = lab.copy()
    lab[BEGIN:END:5] = 200
    lab[BEGIN + 1] = 7
    for mkind in ("none", "two"):
        ref = run_softmax(ctx, x, lab, R.mask_of(mkind), "benign", f"softmax label 200 mask {mkind}")
        assert ref.clamp.sum() == (lab[ref.rows] >= 7).sum() > 5


@pytest.mark.parametrize("Cn", R.SIGMOID_CLS)
def test_sigmoid_head(ctx, Cn):
    for fam in R.SIGMOID_FAMILIES:
        x, y = R.sigmoid_family(fam, Cn)
        for mkind in R.MASKS:
            mk = R.mask_of(mkind)
            what = f"sigmoid {fam} C={Cn} mask {mkind}"
            ref = R.sigmoid_xent(x, y, BEGIN, END, mk)
            other = np.setdiff1d(np.arange(N), ref.rows)
            outside = np.setdiff1d(other, ref.zero_rows)
            probs, loss, diff = canary(N * Cn), canary(N), canary(N * Cn)
            yd, mkd = dev(y), (dev(mk) if mk is not None else None)
            ctx.sigmoid_xent(dev(nan_outside(x, ref.rows)), yd, loss[:N], probs[:N * Cn].view(N, Cn), BEGIN, END, masks=mkd)
            pb, lb = bits(probs), bits(loss)
            untouched(pb[N * Cn:], what + " probabilities, past the end")
            untouched(lb[N:], what + " loss, past the end")
            pb = pb[:N * Cn].reshape(N, Cn)
            untouched(pb[other], what + " probabilities")
            untouched(lb[outside], what + " loss")
            assert (lb[ref.zero_rows] == 0).all(), what + ": a row of the range outside the mask reads loss +0.0"
            p, l = f32(pb)[ref.rows], f32(lb[:N])[ref.rows]
            held("sigmoid_p", fam, R.prob_err(p, ref.p), what)
            held("sigmoid_loss", fam, R.loss_err(l, ref.loss, unit=Cn), what)
            assert_close(p, ref.p, what + " probabilities")
            assert_close(l, ref.loss, what + " loss")
            for k, v in R.SIG_KNOWN:  # 0.0 and -0.0: one half; 88.8: 1; -88.8: expf overflows, 0 or a subnormal
                at = np.nonzero(ref.rows == BEGIN + k)[0]
                if len(at):
                    want = {0: 0.5, 1: 0.5, 2: 1.0}.get(k)
                    assert (p[at[0], 0] == want and p[at[0], Cn - 1] == want) if want else 0 <= p[at[0], 0] <= R.P_TINY_ABS, (what, k, v)
            ctx.d_sigmoid_xent(probs[:N * Cn].view(N, Cn), yd, diff[:N * Cn].view(N, Cn), BEGIN, END, masks=mkd)
            db = bits(diff)
            untouched(db[N * Cn:], what + " gradient, past the end")
            db = db[:N * Cn].reshape(N, Cn)
            untouched(db[other], what + " gradient")
            dref = R.d_sigmoid_xent(f32(pb), y, BEGIN, END, mk)
            held("d_sigmoid", fam, R.rel_elem_err(f32(db)[dref.rows], dref.diff, tiny=R.P_NORMAL), what)
    report(f"C={Cn}", ("sigmoid_p", "sigmoid_loss", "d_sigmoid"), R.SIGMOID_FAMILIES)


# ---- the metrics -------------------------------------------------------------------------------------------------------------
def range_and_masks(n):
    begin, end = (0, 1) if n == 1 else (3, n - 2)
    return begin, end, {"none": None, "third": (np.arange(n) % 3 == 0).astype(np.uint8), "two": (np.arange(n) % 3).astype(np.uint8),
                        "zeros": np.zeros(n, np.uint8)}


def nan_out(a, begin, end, mk):
    """NaN wherever the metric must not look"""
    a = np.array(a, np.float32)
    keep = np.zeros(len(a), bool)
    keep[begin:end] = True if mk is None else mk[begin:end] == 1
    a[~keep] = np.nan
    return a


def both_forms(host_fn, dev_fn):
    """the host form's result and the _dev form's, which must have the same bits and write one float"""
    res = canary(1)
    dev_fn(res[:1])
    got, b = np.float32(host_fn()), bits(res)
    untouched(b[1:], "a _dev metric, past its result")
    assert b[0] == got.view(np.uint32), f"_dev form {f32(b[:1])[0]!r}, host form {got!r}"
    return got


@pytest.mark.parametrize("n", R.LOSS_N)
def test_masked_avg_loss(ctx, n):
    rng = np.random.default_rng(n)
    begin, end, masks = range_and_masks(n)
    ints = rng.integers(0, 16, n).astype(np.float32)
    for mkind, mk in masks.items():
        avg, s, c, _ = R.masked_avg_loss(ints, begin, end, mk)
        ld, mkd = dev(nan_out(ints, begin, end, mk)), (dev(mk) if mk is not None else None)
        got = both_forms(lambda: ctx.masked_avg_loss(ld, begin, end, masks=mkd), lambda r: ctx.masked_avg_loss_dev(ld, begin, end, r, masks=mkd))
        # every partial sum is an integer below 2^24: exact in any order; one correctly rounded division.  No row: 0
        assert got.view(np.uint32) == R.ratio32(s, c).view(np.uint32), (mkind, got, s, c)
        assert mkind != "zeros" or (c == 0 and got.view(np.uint32) == 0)
    if n != max(R.LOSS_N):
        return
    # real losses.  masked_loss_partial_kernel: a thread adds its elements (the range over nblocks x 256 threads, nblocks capped
    # at 1024), wave_sum adds 6 times, thread 0 adds the 4 wave sums (3), finish_partial adds the nblocks block sums: a chain
    # of  per_thread + 6 + 3 + nblocks  additions at most, each off by 2^-24 of a partial sum <= sum |l|; the first addition
    # of a thread and of the host loop add to 0 exactly, which pays for the final division's rounding.  The count is exact.
    nblocks = min(1024, -(-(end - begin) // 256))
    per_thread = -(-(end - begin) // (nblocks * 256))
    assert nblocks == 1024 and per_thread == 2
    chain = per_thread + 6 + 3 + nblocks
    real = (3.0 * rng.standard_normal(n)).astype(np.float32)
    for mkind in ("none", "third"):
        mk = masks[mkind]
        avg, s, c, mag = R.masked_avg_loss(real, begin, end, mk)
        ld, mkd = dev(nan_out(real, begin, end, mk)), (dev(mk) if mk is not None else None)
        got = both_forms(lambda: ctx.masked_avg_loss(ld, begin, end, masks=mkd), lambda r: ctx.masked_avg_loss_dev(ld, begin, end, r, masks=mkd))
        print(f"  masked_avg_loss n={n} mask {mkind}: |got - fp64| {abs(got - avg):.2e}, bound {chain * R.U * mag / c:.2e} (chain {chain})")
        assert abs(np.float64(got) - avg) <= chain * R.U * mag / c


@pytest.mark.parametrize("n,Cn", [(n, Cn) for n in R.LOSS_N[:-1] for Cn in (1, 2, 7, 65)] + [(R.LOSS_N[-1], 2)])
def test_masked_accuracy(ctx, n, Cn):
    begin, end, masks = range_and_masks(n)
    preds, lab = R.tie_preds(n, Cn)
    labd = dev(lab)
    for mkind, mk in masks.items():
        hits, cnt = R.masked_accuracy(preds, lab, begin, end, mk)
        pd_ = preds.copy()
        keep = np.zeros(n, bool)
        keep[begin:end] = True if mk is None else mk[begin:end] == 1
        pd_[~keep] = np.inf if mkind == "third" else np.nan  # (+inf outside would win every comparison it is wrongly part of)
        pd_, mkd = dev(pd_), (dev(mk) if mk is not None else None)
        got = both_forms(lambda: ctx.masked_accuracy_single(pd_, labd, begin, end, masks=mkd),
                         lambda r: ctx.masked_accuracy_single_dev(pd_, labd, begin, end, r, masks=mkd))
        assert got.view(np.uint32) == R.ratio32(hits, cnt).view(np.uint32), (mkind, got, hits, cnt)
    if n >= 255:
        hits, cnt = R.masked_accuracy(preds, lab, begin, end, None)
        assert 0 < hits < cnt  # ties, -inf and NaN rows on both sides of the count


@pytest.mark.parametrize("n,Cn", [(n, Cn) for n in (1, 255, 257, 1023) for Cn in (1, 7, 65)])
def test_f1_counts(ctx, n, Cn):
    rng = np.random.default_rng([n, Cn])
    begin, end, masks = range_and_masks(n)
    pr = rng.choice(np.float32([0.5, np.nan, 0.2, 0.8, np.nextafter(np.float32(0.5), np.float32(1))]), (n, Cn))
    y = rng.integers(0, 3, (n, Cn)).astype(np.uint8)
    prd, yd = dev(pr), dev(y)
    ranges = [(begin, end, mk) for mk in masks.values()] + [(begin, begin, None), (n, n, masks["third"])]
    for b, e, mk in ranges:
        want = R.f1_counts(pr, y, b, e, mk)
        mkd = dev(mk) if mk is not None else None
        f1, cnt = ctx.masked_f1_micro(prd, yd, b, e, masks=mkd)
        assert cnt == want, (b, e, cnt, want)
        assert np.float32(f1).view(np.uint32) == R.f1_micro(*want).view(np.uint32)
        dc = torch.full((3 + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        capi._check(ctx.lib.gaib_masked_f1_counts_dev(ctx.h, b, e, Cn, capi._ptr(mkd), capi._ptr(prd), capi._ptr(yd), capi._ptr(dc)),
                    "gaib_masked_f1_counts_dev")
        dc = dc.cpu().numpy()
        assert tuple(int(k) for k in dc[:3]) == want and (dc[3:] == 0x5A5A5A5A5A5A5A5A).all()
        if b == e:
            assert want == (0, 0, 0) and f1 == 0.0


# ---- l2norm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", R.L2_DIMS)
def test_l2norm(ctx, dim):
    for n in R.L2_ROWS:
        x, g, kind = R.l2_family(n, dim)
        what = f"l2norm n={n} dim={dim}"
        xd, gd, out, dg = dev(x), dev(g), canary(n * dim), canary(n * dim)
        ctx.l2norm(xd, out[:n * dim].view(n, dim))
        ctx.d_l2norm(xd, gd, dg[:n * dim].view(n, dim))
        ob, db = bits(out), bits(dg)
        untouched(ob[n * dim:], what + ", past the last row")
        untouched(db[n * dim:], what + " backward, past the last row")
        got, dgot = f32(ob[:n * dim]).reshape(n, dim), f32(db[:n * dim]).reshape(n, dim)
        ref, dref, top = R.l2norm(x), R.d_l2norm(x, g), R.d_l2norm_scale(x, g)
        for k, fam in enumerate(R.L2_FAMILIES):
            rows = kind == k
            if rows.any():
                held("l2norm", fam, R.rel_elem_err(got[rows], ref[rows]), what)
                held("d_l2norm", fam, R.row_err(dgot[rows], dref[rows], top[rows]), what)
        assert_close(got, ref, what)
    report(f"dim={dim}", ("l2norm", "d_l2norm"), R.L2_FAMILIES)


# ---- Adam ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_one_step(ctx, n):
    alpha = 0.01
    for t in R.ADAM_T:
        p1, p2 = R.beta_powers(t)
        for state in R.ADAM_STATES:
            W0, m0, v0 = R.adam_state(state, n)
            for fam in R.ADAM_GRADS:
                if n > 4099 and fam != "mixed" and (t, state) != (10, "warm"):
                    continue  # above the grid cap: every gradient family once, the mixture at every step and state
                what = f"adam n={n} t={t} state {state} gradient {fam}"
                g = R.adam_grad(fam, n)
                ref = R.adam(W0, m0, v0, g, alpha, p1, p2)
                gd = dev(g)
                a = [canary(n, s) for s in (W0, m0, v0)]
                b = [canary(n, s) for s in (W0, m0, v0)]
                pw = canary(2, [p1, p2])
                ctx.adam_step(gd, a[0][:n], a[1][:n], a[2][:n], alpha, float(p1), float(p2))
                ctx.adam_step_dev(gd, b[0][:n], b[1][:n], b[2][:n], alpha, pw[:2])
                ab, bb = [bits(s) for s in a], [bits(s) for s in b]
                for k, name in enumerate(("W", "m", "v")):
                    untouched(ab[k][n:], f"{what} {name}, past the end")
                    assert np.array_equal(ab[k], bb[k]), f"{what}: adam_step_dev's {name} is not adam_step's"
                pb = bits(pw)
                untouched(pb[2:], what + " beta powers, past the end")
                if t < 5000:  # advanced once, the host's fp32 products
                    assert np.array_equal(pb[:2], bits([p1 * np.float32(0.9), p2 * np.float32(0.999)])), what
                else:
                    assert f32(pb[:1])[0] <= p1 and pb[1] == bits([p2 * np.float32(0.999)])[0]
                W, m, v = (f32(s[:n]) for s in ab)
                held("adam_m", fam, R.scaled_err(m, ref.m, ref.m_scale), what)
                held("adam_v", fam, R.scaled_err(v, ref.v, ref.v), what)
                W64 = W0.astype(np.float64)
                allow = 1.01 * R.U * np.maximum(np.abs(W64), np.abs(W64 + ref.upd))  # the rounding of the store into W
                held("adam_upd", fam, R.scaled_err(W.astype(np.float64) - W64, ref.upd, ref.upd_scale, allow), what)
    report(f"n={n}", ("adam_m", "adam_v", "adam_upd"), R.ADAM_GRADS)


def test_adam_dev_advances_the_powers_of_an_empty_buffer(ctx):
    pw = canary(2, [0.9, 0.999])
    e = torch.empty(0, device="cuda")
    ctx.adam_step_dev(e, e, e, e, 0.01, pw[:2])
    pb = bits(pw)
    untouched(pb[2:], "beta powers, past the end")
    assert np.array_equal(pb[:2], bits([np.float32(0.9) * np.float32(0.9), np.float32(0.999) * np.float32(0.999)]))


# ---- relu ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.RELU_N)
def test_relu_special_values(ctx, n):
    x, g = R.relu_data(n)
    want, dwant = bits(R.relu(x)), bits(R.d_relu(g, x))
    for off in (0, 1):  # 1: every pointer 4 bytes past a 16-byte boundary, the scalar path
        xd, gd = canary(n + off), canary(n + off)
        xd[off:off + n], gd[off:off + n] = dev(x), dev(g)
        assert xd[off:].data_ptr() % 16 == 4 * off
        out, dout = canary(n + off), canary(n + off)
        ctx.relu(xd[off:off + n], out[off:off + n])
        ctx.d_relu(gd[off:off + n], xd[off:off + n], dout[off:off + n])
        for got, w, what in ((bits(out), want, "relu"), (bits(dout), dwant, "d_relu")):
            assert np.array_equal(got[off:off + n], w), f"{what} n={n} offset {off}"
            untouched(got[:off], what + ", before the start")
            untouched(got[off + n:], what + ", past the end")
        ctx.d_relu(gd[off:off + n], xd[off:off + n], gd[off:off + n])  # in place: the gradient
        ctx.relu(xd[off:off + n], xd[off:off + n])  # in place
        for got, w, what in ((bits(xd), want, "relu in place"), (bits(gd), dwant, "d_relu in place")):
            assert np.array_equal(got[off:off + n], w), f"{what} n={n} offset {off}"
            untouched(got[off + n:], what + ", past the end")


# ---- bias_add, colsum, fill, scale ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,length", R.ROWS_COLS)
def test_bias_add_and_colsum(ctx, n, length):
    rng = np.random.default_rng([n, length])
    # colsum_partial_kernel: block b adds its rows_per_block rows of a column one after the other, colsum_finish_kernel the
    # nblocks block sums: a chain of rows_per_block + nblocks additions, each off by 2^-24 of a partial sum <= sum |x[:, j]|
    nblocks = min(1024, (n + 63) // 64)
    rpb = -(-n // nblocks)
    nblocks = -(-n // rpb)
    chain = rpb + nblocks
    for kind in ("integers", "gaussian"):
        x = rng.integers(-8, 9, (n, length)).astype(np.float32) if kind == "integers" else rng.standard_normal((n, length)).astype(np.float32)
        b = rng.integers(-8, 9, length).astype(np.float32) if kind == "integers" else rng.standard_normal(length).astype(np.float32)
        what = f"{kind} {n}x{length}"
        xd, a = canary(n * length, x), canary(length)
        ctx.colsum(xd[:n * length].view(n, length), a[:length])
        ab = bits(a)
        untouched(ab[length:], "colsum " + what + ", past the end")
        got, want = f32(ab[:length]).astype(np.float64), x.astype(np.float64).sum(0)
        if kind == "integers":  # every partial sum an integer below 2^24
            assert np.array_equal(got, want), "colsum " + what
        else:
            lim = chain * R.U * np.abs(x.astype(np.float64)).sum(0)
            print(f"  colsum {what}: worst |got - fp64| / bound {float((np.abs(got - want) / lim).max()):.2e} (chain {chain})")
            assert (np.abs(got - want) <= lim).all(), "colsum " + what
        ctx.bias_add(xd[:n * length].view(n, length), dev(b))
        xb = bits(xd)
        untouched(xb[n * length:], "bias_add " + what + ", past the end")
        assert np.array_equal(xb[:n * length].reshape(n, length), bits(x + b[None, :])), "bias_add " + what  # one fp32 addition


def test_colsum_of_no_rows_writes_zeros(ctx):
    for length in (1, 47, 300):
        a = canary(length)
        ctx.colsum(torch.empty(0, length, device="cuda"), a[:length])
        ab = bits(a)
        assert (ab[:length] == 0).all()
        untouched(ab[length:], "colsum of no rows, past the end")


@pytest.mark.parametrize("n", R.FLAT_N)
def test_fill_and_scale(ctx, n):
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    xd = canary(n, x)
    capi._check(ctx.lib.gaib_scale_f32(ctx.h, n, -1.7, capi._ptr(xd)), "gaib_scale_f32")
    xb = bits(xd)
    untouched(xb[n:], "scale, past the end")
    assert np.array_equal(xb[:n], bits(np.float32(-1.7) * x))
    capi._check(ctx.lib.gaib_fill_f32(ctx.h, n, 2.5, capi._ptr(xd)), "gaib_fill_f32")
    xb = bits(xd)
    untouched(xb[n:], "fill, past the end")
    assert (f32(xb[:n]) == 2.5).all()


# ---- sgemm with a dimension of 0 -------------------------------------------------------------------------------------------------
def test_sgemm_with_a_dimension_of_zero(ctx):
    M, Nn = 5, 7
    c0, _ = R.relu_data(M * Nn)  # NaN, +-0, +-inf, subnormals
    A, B = torch.empty(M, 0, device="cuda"), torch.empty(0, Nn, device="cuda")
    for accum, relu, want in ((False, False, np.zeros(M * Nn, np.float32)), (True, False, c0), (True, True, R.relu(c0)),
                              (False, True, np.zeros(M * Nn, np.float32))):
        Cm = canary(M * Nn, c0)
        ctx.sgemm(A, B, Cm[:M * Nn].view(M, Nn), accum=accum, relu=relu)
        cb = bits(Cm)
        untouched(cb[M * Nn:], "sgemm K = 0, past the end")
        assert np.array_equal(cb[:M * Nn], bits(want)), f"sgemm K = 0 accumulate {accum} relu {relu}"
    X = dev(np.ones((4, 3), np.float32))
    for m, nn in ((0, Nn), (M, 0), (0, 0)):
        for flags in (0, 1, 3):
            Cm = canary(8)
            capi._check(ctx.lib.gaib_sgemm_ex(ctx.h, 0, 0, m, nn, 3, capi._ptr(X), capi._ptr(X), flags, capi._ptr(Cm)), "gaib_sgemm_ex")
            untouched(bits(Cm), f"sgemm M = {m}, N = {nn}")
