"""The inputs of the head tests (tests/head_ref64.py) and the fp32 oracle on them, without a GPU: every family keeps what it
promises (the asserts of the family functions), head_ref64 agrees with independent dense formulas, and the oracle stays within
head_ref64.ORACLE_DIST of the fp64 reference on every family and shape -- the figures the GPU tests
(tests/test_gpu_head_extremes.py) multiply by GPU_FACTOR.  Each test prints what it measured (pytest -s).

Where the oracle is not the yardstick:
  * a range whose mask holds no row: the oracle's accuracy is 0 / 0; the library returns 0 for both metrics;
  * d_l2norm on the 1e15 rows: the reference's powf(sum, -1.5) is below the smallest fp32 subnormal from a sum of squares of
    about 8e29 on, so the oracle returns rows of 0 where the gradient is about 1e-17 (asserted here as what it does); the
    kernel forms the coefficient in two factors there and is held to fp64 like every other row;
  * the oracle has no bias_add / colsum / fill / scale and no sgemm at K = 0."""
import ctypes as C

import numpy as np
import pytest

import head_ref64 as R
from oracle import binding as orc

BEGIN, END, N = R.HEAD_BEGIN, R.HEAD_END, R.HEAD_N
SEEN = {}


def held(op, family, value):
    """record the oracle's distance; it must stay at the constant the GPU bound is made from -- with a quarter of headroom here
    (not in the GPU bound): glibc picks its expf / logf / powf by CPU, and another variant may round a few results the other way"""
    SEEN[(op, family)] = max(SEEN.get((op, family), 0.0), value)
    assert value <= 1.25 * R.ORACLE_DIST[(op, family)], f"{op} {family}: oracle {value:.3e}, recorded {R.ORACLE_DIST[(op, family)]:.3e}"


def report(head, op, families):
    """the worst distances so far"""
    print(f"  {head} {op}: " + "  ".join(f"{f} {SEEN.get((op, f), 0.0):.2e}" for f in families))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_reference_against_dense_formulas():
    """softmax: log p = x - logsumexp(x), the loss -log p[label], the gradient the derivative of the summed loss by finite
    differences; sigmoid: the loss max(x, 0) - x y + log1p(exp(-|x|)), p = the derivative of the loss by x plus y"""
    rng = np.random.default_rng(5)
    n, Cn, b, e = 12, 9, 2, 11
    x = (4 * rng.standard_normal((n, Cn))).astype(np.float32)
    lab = rng.integers(0, Cn, n).astype(np.uint8)
    mask = (np.arange(n) % 3).astype(np.uint8)  # 0, 1, 2
    for mk in (None, mask):
        ref = R.softmax_xent(x, lab, b, e, mk)
        assert np.array_equal(ref.rows, [i for i in range(b, e) if mk is None or mk[i] == 1])
        xs = x[ref.rows].astype(np.float64)
        lse = np.log(np.exp(xs - xs.max(1, keepdims=True)).sum(1)) + xs.max(1)
        assert np.allclose(np.log(ref.p), xs - lse[:, None], rtol=0, atol=1e-13)
        assert np.allclose(ref.loss, lse - xs[np.arange(len(xs)), lab[ref.rows]], rtol=1e-13, atol=1e-13)
        full = np.zeros((n, Cn))  # (p is [rows]: the backward takes the whole array)
        full[ref.rows] = ref.p
        d = R.d_softmax_xent(full, lab, b, e, mk)
        total = lambda z: R.softmax_xent(z, lab, b, e, mk).loss.sum() / (e - b)  # noqa: E731
        for i, j in ((ref.rows[0], 0), (ref.rows[-1], Cn - 1), (ref.rows[1], int(lab[ref.rows[1]]))):
            z = x.astype(np.float64)
            zp, zm = z.copy(), z.copy()
            zp[i, j] += 1e-6
            zm[i, j] -= 1e-6
            assert abs((total(zp) - total(zm)) / 2e-6 - d.diff[list(d.rows).index(i), j]) < 1e-9
    y = (rng.random((n, Cn)) < 0.4).astype(np.uint8)
    x[3, 0], x[3, 1], x[4, 0] = 0.0, -0.0, 88.8
    for mk in (None, mask):
        ref = R.sigmoid_xent(x, y, b, e, mk)
        xs, ys = x[ref.rows].astype(np.float64), y[ref.rows].astype(np.float64)
        dense = np.maximum(xs, 0) - xs * ys + np.log1p(np.exp(-np.abs(xs)))
        assert np.allclose(ref.terms, dense, rtol=1e-14, atol=1e-300) and (ref.terms >= 0).all()
        assert np.allclose(ref.loss, dense.sum(1), rtol=1e-13)
        assert np.allclose(ref.p, 0.5 * (1 + np.tanh(xs / 2)), rtol=1e-13)
        assert set(ref.rows) | set(ref.zero_rows) == set(range(b, e)) and not set(ref.rows) & set(ref.zero_rows)
    # the clamp: a label 120 below the maximum, and a label that is no class
    z = np.zeros((3, 4), np.float32)
    z[0, 1] = -120.0
    ref = R.softmax_xent(z, np.array([1, 0, 200], np.uint8), 0, 3)
    assert list(ref.clamp) == [True, False, True] and ref.loss[0] == np.float64(R.CLAMP32) and abs(ref.loss[1] - np.log(4)) < 1e-15
    # l2norm: unit rows, the gradient orthogonal to x, a clamped row scales by 1e6 / 1e6
    xl, gl, kind = R.l2_family(7, 65)
    out, dg = R.l2norm(xl), R.d_l2norm(xl, gl)
    live = kind % 4 != 1
    assert np.allclose((out[kind == 0] ** 2).sum(1), 1) and np.allclose((out[kind == 3] ** 2).sum(1), 1) and not out[kind == 1].any()
    assert np.allclose(out[kind == 2], xl[kind == 2].astype(np.float64) * 1e6)
    assert np.allclose(dg[kind == 1], gl[kind == 1].astype(np.float64) * 1e6)  # x = 0: g s2 c1 = g / sqrt(1e-12)
    full = (kind == 0) | (kind == 3)
    assert (np.abs((dg[full] * xl[full]).sum(1)) <= 1e-12 * np.abs(dg[full] * xl[full]).sum(1)).all() and live.any()
    # Adam at t = 1 from the zero state: the step is alpha g / sqrt(g^2 + eps)
    g = R.adam_grad("small", 257)
    a = R.adam(np.zeros(257), np.zeros(257), np.zeros(257), g, 0.01, 0.9, 0.999)
    g64 = g.astype(np.float64)
    assert np.allclose(a.upd, -0.01 * g64 / np.sqrt(g64 ** 2 + np.float64(np.float32(1e-8))), rtol=1e-6)
    # eps inside the root decides: |step| / alpha runs from 1e-6 / 1e-4 to 1e-4 / sqrt(2e-8), never 1 as with eps outside
    assert 0.0099 < (np.abs(a.upd) / 0.01).min() and (np.abs(a.upd) / 0.01).max() < 0.7072
    # b1^5000: the fp32 products end at four subnormal steps (0.9 x 4 rounds back to 4) or, flushed, at 0: 1 - b1^t is 1
    p1, p2 = R.beta_powers(5000)
    assert p1 < np.float32(1e-44) and np.float32(1) - p1 == 1 and 0 < p2 < 0.01


# ---- the loss heads ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", R.SOFTMAX_CLS)
def test_softmax_oracle(Cn):
    for fam in R.SOFTMAX_FAMILIES:
        x, lab = R.softmax_family(fam, Cn)
        for mkind in R.MASKS:
            mk = R.mask_of(mkind)
            ref = R.softmax_xent(x, lab, BEGIN, END, mk)
            p, loss = orc.softmax_xent_fwd(x, lab, BEGIN, END, mk)
            held("softmax_p", fam, R.prob_err(p[ref.rows], ref.p, ref.xm))
            held("softmax_loss", fam, R.loss_err(loss[ref.rows], ref.loss))
            assert np.array_equal(bits(loss[ref.rows][ref.clamp]), bits(np.full(int(ref.clamp.sum()), R.CLAMP32))), (fam, mkind)
            if fam == "clamp" and Cn > 1:
                assert ref.clamp.all()
            dref = R.d_softmax_xent(p, lab, BEGIN, END, mk)
            d = orc.softmax_xent_bwd(p, lab, BEGIN, END, mk)
            held("d_softmax", fam, R.rel_elem_err(d[dref.rows], dref.diff, tiny=R.P_NORMAL))
    for op in ("softmax_p", "softmax_loss", "d_softmax"):
        report(f"C={Cn}", op, R.SOFTMAX_FAMILIES)


@pytest.mark.parametrize("Cn", R.SIGMOID_CLS)
def test_sigmoid_oracle(Cn):
    for fam in R.SIGMOID_FAMILIES:
        x, y = R.sigmoid_family(fam, Cn)
        for mkind in R.MASKS:
            mk = R.mask_of(mkind)
            ref = R.sigmoid_xent(x, y, BEGIN, END, mk)
            p, loss = orc.sigmoid_xent_fwd(x, y, BEGIN, END, mk)
            held("sigmoid_p", fam, R.prob_err(p[ref.rows], ref.p))
            held("sigmoid_loss", fam, R.loss_err(loss[ref.rows], ref.loss, unit=Cn))
            dref = R.d_sigmoid_xent(p, y, BEGIN, END, mk)
            d = orc.sigmoid_xent_bwd(p, y, BEGIN, END, mk)
            held("d_sigmoid", fam, R.rel_elem_err(d[dref.rows], dref.diff, tiny=R.P_NORMAL))
    for op in ("sigmoid_p", "sigmoid_loss", "d_sigmoid"):
        report(f"C={Cn}", op, R.SIGMOID_FAMILIES)


# ---- the metrics -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.LOSS_N)
def test_metrics_oracle(n):
    rng = np.random.default_rng(n)
    begin, end = (0, 1) if n == 1 else (3, n - 2)
    ints = rng.integers(0, 16, n).astype(np.float32)
    masks = {"none": None, "third": (np.arange(n) % 3 == 0).astype(np.uint8), "two": (np.arange(n) % 3).astype(np.uint8)}
    for mk in masks.values():
        avg, s, c, _ = R.masked_avg_loss(ints, begin, end, mk)
        if c:
            assert np.float32(orc.masked_avg_loss(ints, begin, end, mk)) == R.ratio32(s, c)  # integer sums: exact in any order
    real = rng.exponential(2.0, n).astype(np.float32)
    avg, s, c, mag = R.masked_avg_loss(real, begin, end, None)
    assert abs(orc.masked_avg_loss(real, begin, end, None) - avg) <= (c + 1) * R.U * mag / c  # a chain of c additions, one division
    assert R.masked_avg_loss(real, begin, end, np.zeros(n, np.uint8))[:3] == (0.0, 0.0, 0)
    if n <= 1023:
        for Cn in (1, 2, 7, 65):
            preds, lab = R.tie_preds(n, Cn)
            for mk in masks.values():
                hits, cnt = R.masked_accuracy(preds, lab, begin, end, mk)
                if cnt:
                    assert np.float32(orc.masked_accuracy_single(preds, lab, begin, end, mk)) == R.ratio32(hits, cnt)
            # F1: 0.5 exactly, NaN, label bytes of 2
            pr = rng.choice(np.float32([0.5, np.nan, 0.2, 0.8, 0.50000006]), (n, Cn))
            y = rng.integers(0, 3, (n, Cn)).astype(np.uint8)
            for mk in masks.values():
                f1, cnt3 = orc.masked_f1_micro(pr, y, begin, end, mk, return_counts=True)
                assert tuple(int(k) for k in cnt3) == R.f1_counts(pr, y, begin, end, mk)
                assert np.float32(f1) == R.f1_micro(*cnt3)
        assert R.f1_counts(pr, y, 2, 2) == (0, 0, 0) and R.f1_micro(0, 0, 0) == 0


# ---- l2norm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", R.L2_DIMS)
def test_l2norm_oracle(dim):
    for n in R.L2_ROWS:
        x, g, kind = R.l2_family(n, dim)
        out, dg = orc.l2norm(x), orc.d_l2norm(x, g)
        ref, dref, top = R.l2norm(x), R.d_l2norm(x, g), R.d_l2norm_scale(x, g)
        for k, fam in enumerate(R.L2_FAMILIES):
            rows = kind == k
            if not rows.any():
                continue
            held("l2norm", fam, R.rel_elem_err(out[rows], ref[rows]))
            if fam == "large":
                # powf(sum, -1.5) underflows: the oracle returns 0 where the terms are ~1e-17 (dim = 1: one subnormal step
                # times two terms that cancel)
                assert (np.abs(dg[rows]).max(1) <= 1e-6 * top[rows]).all()
            else:
                held("d_l2norm", fam, R.row_err(dg[rows], dref[rows], top[rows]))
    report(f"dim={dim}", "l2norm", R.L2_FAMILIES)
    report(f"dim={dim}", "d_l2norm", R.L2_FAMILIES)


# ---- Adam ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_oracle(n):
    alpha = 0.01
    for t in R.ADAM_T:
        p1, p2 = R.beta_powers(t)
        for state in R.ADAM_STATES:
            W0, m0, v0 = R.adam_state(state, n)
            for fam in R.ADAM_GRADS:
                g = R.adam_grad(fam, n)
                ref = R.adam(W0, m0, v0, g, alpha, p1, p2)
                W, m, v = W0.copy(), m0.copy(), v0.copy()
                b1_t, b2_t = C.c_float(p1), C.c_float(p2)
                orc.lib().orc_adam_update(C.c_int64(n), orc._p(g), orc._p(W), orc._p(m), orc._p(v), C.c_float(alpha),
                                          C.byref(b1_t), C.byref(b2_t))
                assert np.float32(b1_t.value) == np.float32(p1 * np.float32(0.9)) and np.float32(b2_t.value) == np.float32(p2 * np.float32(0.999))
                held("adam_m", fam, R.scaled_err(m, ref.m, ref.m_scale))
                held("adam_v", fam, R.scaled_err(v, ref.v, ref.v))
                W64 = W0.astype(np.float64)
                allow = 1.01 * R.U * np.maximum(np.abs(W64), np.abs(W64 + ref.upd))  # the rounding of the store into W
                held("adam_upd", fam, R.scaled_err(W.astype(np.float64) - W64, ref.upd, ref.upd_scale, allow))
    for op in ("adam_m", "adam_v", "adam_upd"):
        report(f"n={n}", op, R.ADAM_GRADS)


# ---- relu ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.RELU_N)
def test_relu_oracle(n):
    x, g = R.relu_data(n)
    assert np.array_equal(bits(orc.relu(x)), bits(R.relu(x)))
    assert np.array_equal(bits(orc.d_relu(g, x)), bits(R.d_relu(g, x)))
    if n > 12:
        assert np.isnan(x).any() and np.isinf(x).any() and (bits(x) == 0x80000000).any() and (np.abs(x[x != 0]) < 1e-38).any()
        assert not np.isnan(R.relu(x)).any() and (bits(R.relu(x))[bits(x) == 0x80000000] == 0).all()
