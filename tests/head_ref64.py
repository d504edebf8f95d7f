"""The loss heads, the masked metrics, l2norm, Adam and the dense helpers in fp64 (numpy, host only), and the input families of
tests/test_head_extremes_cpu.py and tests/test_gpu_head_extremes.py.

Every function restates the operation as the library defines it (csrc/elementwise.hip, oracle/gnn_oracle.c), quirks included:
  * masks[i] == 1 alone is "in" (a mask byte of 2 is "out");
  * the softmax backward divides by end - begin, not by the number of rows in the mask;
  * a softmax row outside the mask keeps everything; a sigmoid row of the range outside the mask reads loss 0 and keeps its
    probabilities;
  * the softmax loss of a label whose fp32 probability is exactly 0 (below 2^-150 here), or whose label is no class at all, is
    CLAMP32 = -logf(1e-10f);
  * accuracy takes the first maximum, best = -1 where nothing exceeds -inf (a row of -inf or NaN never hits);
  * F1 counts pred > 0.5 as hot, pred <= 0.5 as cold (a NaN prediction is neither) and only label bytes 0 and 1;
  * l2norm clamps the sum of squares at 1e-12, forward and backward;
  * Adam has eps inside the root, and the beta powers are inputs.
Inputs are the fp32 arrays the kernels get, widened: the reference never sees a value the kernel does not see.

ORACLE_DIST holds the fp32 oracle's worst distance from these references per operation and family, measured by
tests/test_head_extremes_cpu.py (which asserts them); the GPU tests allow GPU_FACTOR times as much.  The GPU's own figures
stand beside them in LEDGER 22."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

CLAMP32 = np.float32(-np.log(np.float32(1e-10)))
P_ZERO = 2.0 ** -150  # a probability below this rounds to +0.0f (half of the smallest subnormal)
P_NORMAL = 2.0 ** -125  # twice the smallest normal fp32: at or above it both sides are normal numbers
P_TINY_ABS = 2.0 ** -126  # below P_NORMAL an fp32 result may be subnormal or flushed: |got - ref| <= the smallest normal
U = 2.0 ** -24  # the unit roundoff of fp32
GPU_FACTOR = 4.0

# ---- the shapes ---------------------------------------------------------------------------------------------------------------
HEAD_N, HEAD_BEGIN, HEAD_END = 203, 5, 198  # 193 rows: the last block of 4 is partial, begin is no multiple of 4
SOFTMAX_CLS = (1, 2, 7, 63, 64, 65, 128, 129, 172, 255)
SIGMOID_CLS = (1, 63, 64, 65, 121, 200)
SOFTMAX_FAMILIES = ("benign", "offset", "wide", "clamp", "ties", "spike")
SIGMOID_FAMILIES = ("benign", "offset", "wide", "ties", "spike", "scale100", "scale1e4")
MASKS = ("none", "third", "zeros", "ones", "two")
L2_DIMS = (1, 3, 63, 64, 65, 127, 128, 129, 200, 1000)
L2_ROWS = (1, 5, 7, 64)
L2_FAMILIES = ("benign", "zero", "tiny", "large")
ADAM_N = (1, 255, 257, 4099, 524288 + 4099)  # the last: above the grid cap of 2048 x 256
ADAM_T = (1, 10, 5000)
ADAM_GRADS = ("normal", "small", "zero", "huge", "mixed")
ADAM_STATES = ("zero", "warm")
RELU_N = (1, 3, 5, 4097)
ROWS_COLS = ((1, 1), (63, 47), (64, 300), (65, 257), (4097, 100), (70001, 7))
LOSS_N = (1, 255, 256, 257, 1023, 262144 + 257)
FLAT_N = (0, 1, 524288 + 3)

# ---- the fp32 oracle's worst distance from this file, by metric (measured on the CPU, asserted by the CPU test; the GPU gets
# GPU_FACTOR times each).  Beside each: what the MI355X kernels measured (LEDGER 22).
# softmax probabilities: |got - ref| / (ref (1 + |x - max|)) over ref >= P_NORMAL
# softmax loss: |got - ref| / (1 + |ref|);  sigmoid loss: |got - ref| / (num_cls + |ref|)  (see *_err below)
# d_softmax, d_sigmoid, l2norm: element-wise relative; d_l2norm: row-wise in units of d_l2norm_scale
# adam_m / adam_v / adam_upd: in units of m_scale / v' / upd_scale, the update after the rounding of the store into W
# A figure of 0 is an operation that is exact on that family (probabilities of exactly 0, 1/2 and 1): the kernels must be too.
#
# The kernels on an MI355X, the worst over shapes and masks, in the order of the entries below (every one under its oracle
# figure except sigmoid_p, 1.04e-7 against 8.9e-8, and d_l2norm `large`, which the oracle does not measure):
#   softmax_p     2.0e-7  2.4e-7  2.2e-7  2.2e-7  1.8e-7  0          softmax_loss  1.6e-7  1.2e-7  1.3e-7  0  1.3e-7  0
#   d_softmax     5.9e-8 (spike 2.5e-8)                              sigmoid_p     9.9e-8  0  1.0e-7  4.0e-8  0  1.0e-7  8.7e-8
#   sigmoid_loss  7.9e-8  1.1e-7  1.2e-7  7.7e-8  8.8e-8  1.4e-7  1.5e-7
#   d_sigmoid     1.0e-7  2.5e-8  1.0e-7  5.2e-8  2.5e-8  9.5e-8  6.0e-8
#   l2norm        1.3e-7  0  1.6e-8  5.4e-8                          d_l2norm      1.8e-7  1.1e-7  1.6e-7  1.1e-7
#   adam_m        1.1e-7  1.2e-7  5.7e-8  1.9e-8  1.2e-7             adam_v        1.5e-7  1.1e-7  6.0e-8  2.1e-8  1.4e-7
#   adam_upd      1.7e-7  2.2e-7  1.5e-7  1.3e-8  1.9e-7
ORACLE_DIST = {
    ("softmax_p", "benign"): 8.1e-7, ("softmax_p", "offset"): 7.9e-7, ("softmax_p", "wide"): 4.0e-7,
    ("softmax_p", "clamp"): 9.5e-7, ("softmax_p", "ties"): 2.0e-6, ("softmax_p", "spike"): 0.0,
    ("softmax_loss", "benign"): 2.8e-7, ("softmax_loss", "offset"): 2.4e-7, ("softmax_loss", "wide"): 1.3e-7,
    ("softmax_loss", "clamp"): 0.0, ("softmax_loss", "ties"): 3.5e-7, ("softmax_loss", "spike"): 0.0,
    ("d_softmax", "benign"): 6.0e-8, ("d_softmax", "offset"): 6.0e-8, ("d_softmax", "wide"): 6.0e-8,
    ("d_softmax", "clamp"): 6.0e-8, ("d_softmax", "ties"): 6.0e-8, ("d_softmax", "spike"): 2.6e-8,
    ("sigmoid_p", "benign"): 8.9e-8, ("sigmoid_p", "offset"): 0.0, ("sigmoid_p", "wide"): 8.9e-8, ("sigmoid_p", "ties"): 4.1e-8,
    ("sigmoid_p", "spike"): 0.0, ("sigmoid_p", "scale100"): 8.9e-8, ("sigmoid_p", "scale1e4"): 8.2e-8,
    ("sigmoid_loss", "benign"): 3.9e-7, ("sigmoid_loss", "offset"): 4.8e-7, ("sigmoid_loss", "wide"): 4.6e-7,
    ("sigmoid_loss", "ties"): 8.4e-7, ("sigmoid_loss", "spike"): 4.1e-6, ("sigmoid_loss", "scale100"): 4.5e-7,
    ("sigmoid_loss", "scale1e4"): 3.8e-7,
    ("d_sigmoid", "benign"): 1.1e-7, ("d_sigmoid", "offset"): 2.6e-8, ("d_sigmoid", "wide"): 1.1e-7, ("d_sigmoid", "ties"): 5.2e-8,
    ("d_sigmoid", "spike"): 2.6e-8, ("d_sigmoid", "scale100"): 9.6e-8, ("d_sigmoid", "scale1e4"): 6.1e-8,
    ("l2norm", "benign"): 4.4e-7, ("l2norm", "zero"): 0.0, ("l2norm", "tiny"): 1.7e-8, ("l2norm", "large"): 2.2e-6,
    # `large`: the oracle's powf(sum, -1.5) underflows there (it returns rows of 0), so it measures nothing; the kernel's
    # two-factor form takes the same sums and one division more than the benign rows' form: the benign figure
    ("d_l2norm", "benign"): 4.1e-7, ("d_l2norm", "zero"): 1.2e-7, ("d_l2norm", "tiny"): 1.6e-7, ("d_l2norm", "large"): 4.1e-7,
    ("adam_m", "normal"): 1.2e-7, ("adam_m", "small"): 1.2e-7, ("adam_m", "zero"): 5.7e-8, ("adam_m", "huge"): 2.0e-8,
    ("adam_m", "mixed"): 1.2e-7,
    ("adam_v", "normal"): 1.6e-7, ("adam_v", "small"): 1.2e-7, ("adam_v", "zero"): 6.0e-8, ("adam_v", "huge"): 2.1e-8,
    ("adam_v", "mixed"): 1.5e-7,
    ("adam_upd", "normal"): 2.1e-7, ("adam_upd", "small"): 2.2e-7, ("adam_upd", "zero"): 1.9e-7, ("adam_upd", "huge"): 1.3e-8,
    ("adam_upd", "mixed"): 1.9e-7,
}


def bound(op, family):
    return GPU_FACTOR * ORACLE_DIST[(op, family)]


def _in_rows(n, begin, end, masks):
    rows = np.arange(begin, end)
    if masks is None:
        return rows, rows[:0]
    m = np.asarray(masks)
    return rows[m[begin:end] == 1], rows[m[begin:end] != 1]


# ---- the operations -------------------------------------------------------------------------------------------------------------
def softmax_xent(x, labels, begin, end, masks=None):
    """rows: the rows it defines; p [rows][C], loss [rows], xm = x - max [rows][C], clamp [rows]: the loss is CLAMP32 there"""
    x = np.asarray(x, np.float64)
    rows, _ = _in_rows(len(x), begin, end, masks)
    xr = x[rows]
    xm = xr - xr.max(1, keepdims=True)
    e = np.exp(xm)
    p = e / e.sum(1, keepdims=True)
    lab = np.asarray(labels)[rows].astype(np.int64)
    real = lab < x.shape[1]
    pl = np.where(real, p[np.arange(len(rows)), np.minimum(lab, x.shape[1] - 1)], 0.0)
    clamp = pl < P_ZERO
    with np.errstate(divide="ignore"):
        loss = np.where(clamp, np.float64(CLAMP32), -np.log(pl))
    return SimpleNamespace(rows=rows, p=p, loss=loss, xm=xm, clamp=clamp, pl=pl)


def d_softmax_xent(p, labels, begin, end, masks=None):
    """(p - onehot) / (end - begin) on the rows of the mask; p: the fp32 probabilities handed to the call"""
    p = np.asarray(p, np.float64)
    rows, _ = _in_rows(len(p), begin, end, masks)
    onehot = np.asarray(labels)[rows].astype(np.int64)[:, None] == np.arange(p.shape[1])[None, :]
    return SimpleNamespace(rows=rows, diff=(p[rows] - onehot) / float(end - begin))


def sigmoid_xent(x, labels, begin, end, masks=None):
    """rows: in the mask (p, loss defined); zero_rows: rows of the range outside the mask (loss 0.0, probabilities kept)"""
    x = np.asarray(x, np.float64)
    rows, zero_rows = _in_rows(len(x), begin, end, masks)
    xr, y = x[rows], np.asarray(labels)[rows].astype(np.float64)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-xr))
    pos = (xr >= 0).astype(np.float64)
    terms = -(xr * (y - pos) - np.log1p(np.exp(xr - 2.0 * xr * pos)))
    return SimpleNamespace(rows=rows, zero_rows=zero_rows, p=p, loss=terms.sum(1), terms=terms)


def d_sigmoid_xent(p, labels, begin, end, masks=None):
    p = np.asarray(p, np.float64)
    rows, _ = _in_rows(len(p), begin, end, masks)
    return SimpleNamespace(rows=rows, diff=(p[rows] - np.asarray(labels)[rows].astype(np.float64)) / float(end - begin))


def masked_avg_loss(loss, begin, end, masks=None):
    """(the average, 0 where the mask holds no row of the range; the sum; the count; the sum of magnitudes)"""
    rows, _ = _in_rows(len(loss), begin, end, masks)
    l = np.asarray(loss, np.float64)[rows]
    s, c = float(l.sum()), len(rows)
    return (s / c if c else 0.0), s, c, float(np.abs(l).sum())


def masked_accuracy(preds, labels, begin, end, masks=None):
    """(hits, count): the first maximum above -inf against the label"""
    preds = np.asarray(preds)
    rows, _ = _in_rows(len(preds), begin, end, masks)
    with np.errstate(invalid="ignore"):
        above = preds[rows] > -np.inf  # (NaN and -inf never are)
    best = np.where(above, preds[rows], -np.inf).argmax(1)  # argmax: the first of equal maxima
    best[~above.any(1)] = -1
    return int((best == np.asarray(labels)[rows].astype(np.int64)).sum()), len(rows)


def ratio32(a, b):
    """a / b as one correctly rounded fp32 division of two exactly held integers; 0 for b == 0"""
    return np.float32(0.0) if b == 0 else np.float32(np.float32(a) / np.float32(b))


def f1_counts(preds, labels, begin, end, masks=None):
    preds, labels = np.asarray(preds), np.asarray(labels)
    rows, _ = _in_rows(len(preds), begin, end, masks)
    with np.errstate(invalid="ignore"):
        hot, cold = preds[rows] > 0.5, preds[rows] <= 0.5
    y = labels[rows]
    return int(((y == 1) & hot).sum()), int(((y == 0) & hot).sum()), int(((y == 1) & cold).sum())


def f1_micro(tp, fp, fn):
    prec = tp / (tp + fp) if tp + fp > 0 else 0.0
    rec = tp / (tp + fn) if tp + fn > 0 else 0.0
    return np.float32(2.0 * (rec * prec) / (rec + prec) if rec + prec > 0 else 0.0)


def l2norm(x):
    x = np.asarray(x, np.float64)
    s = np.maximum((x * x).sum(1, keepdims=True), 1e-12)
    return x / np.sqrt(s)


def d_l2norm(x, g):
    """x c0 c1 + g s2 c1 with s2 = max(sum x^2, 1e-12), c0 = -<x, g>, c1 = s2^-1.5"""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    s2 = np.maximum((x * x).sum(1, keepdims=True), 1e-12)
    c0 = -(x * g).sum(1, keepdims=True)
    c1 = s2 ** -1.5
    return x * c0 * c1 + g * s2 * c1


def d_l2norm_scale(x, g):
    """per row, the largest magnitude the two terms of d_l2norm reach, max_j (|x c0 c1| + |g s2 c1|): the row's own scale.  The
    terms cancel (entirely at dim = 1, where the gradient is 0), so the row's largest RESULT would be no scale at all there."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    s2 = np.maximum((x * x).sum(1, keepdims=True), 1e-12)
    c0 = -(x * g).sum(1, keepdims=True)
    return ((np.abs(x * c0) + np.abs(g * s2)) * s2 ** -1.5).max(1)


def adam(W, m, v, g, alpha, b1_t, b2_t, b1=0.9, b2=0.999, eps=1e-8):
    """one step from the fp32 state: m', v', upd = W' - W, and the magnitudes m' and the update are judged in (m_scale,
    upd_scale); every scalar is the fp32 number the call gets"""
    f = lambda a: np.float64(np.float32(a))  # noqa: E731
    m, v, g = (np.asarray(a, np.float64) for a in (m, v, g))
    b1, b2, alpha, eps, b1_t, b2_t = f(b1), f(b2), f(alpha), f(eps), f(b1_t), f(b2_t)
    mt = b1 * m + (1.0 - b1) * g
    vt = b2 * v + (1.0 - b2) * g * g
    mag = np.abs(b1 * m) + np.abs((1.0 - b1) * g)  # what m' was summed from: m and g of opposite sign cancel
    root = np.sqrt(vt / (1.0 - b2_t) + eps)
    return SimpleNamespace(m=mt, v=vt, upd=-alpha * (mt / (1.0 - b1_t)) / root, m_scale=mag,
                           upd_scale=alpha * (mag / (1.0 - b1_t)) / root)


def beta_powers(t, b1=0.9, b2=0.999):
    """(b1^t, b2^t) as the library advances them: t - 1 fp32 products from (b1, b2)"""
    p1, p2 = np.float32(b1), np.float32(b2)
    for _ in range(t - 1):
        p1, p2 = np.float32(p1 * np.float32(b1)), np.float32(p2 * np.float32(b2))
    return p1, p2


def relu(x):
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, np.float32(0.0)).astype(np.float32)


def d_relu(g, data):
    with np.errstate(invalid="ignore"):
        return np.where(data > 0, g, np.float32(0.0)).astype(np.float32)


# ---- error metrics ----------------------------------------------------------------------------------------------------------------
def prob_err(got, ref, xm=None):
    """the worst |got - ref| / (ref (1 + |x - max|)) over ref >= P_NORMAL (rounding the exponent's argument alone contributes
    |x - max| 2^-24); below P_NORMAL the fp32 value may be subnormal or flushed: asserts |got - ref| <= 2^-126 there"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and not np.isnan(got).any()
    big = ref >= P_NORMAL
    assert (np.abs(got - ref)[~big] <= P_TINY_ABS).all(), "a probability below the normal range is off by more than 2^-126"
    w = 1.0 if xm is None else 1.0 + np.abs(np.asarray(xm, np.float64))
    return float((np.abs(got - ref)[big] / (ref * w)[big]).max(initial=0.0))


def loss_err(got, ref, unit=1.0):
    """|got - ref| / (unit + |ref|): -log(p (1 + d)) is off by d whatever the loss, and d grows with 1 + |x - max| <= 1 + loss;
    a sigmoid row sums num_cls terms each off by up to 2^-24 (1 + term): unit = num_cls"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    return float((np.abs(got - ref) / (unit + np.abs(ref))).max(initial=0.0))


def rel_elem_err(got, ref, tiny=0.0):
    """the worst |got - ref| / |ref|; where ref == 0 got must be 0 (+-), entries with |ref| < tiny held to |got - ref| <= tiny"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    small = np.abs(ref) <= tiny
    assert (np.abs(got - ref)[small] <= tiny).all()
    return float((np.abs(got - ref)[~small] / np.abs(ref)[~small]).max(initial=0.0))


def scaled_err(got, ref, scale, allow=0.0):
    """the worst (|got - ref| - allow)+ / scale; where scale == 0 nothing beyond `allow` may be left"""
    got, ref, scale = (np.asarray(a, np.float64) for a in (got, ref, scale))
    over = np.maximum(np.abs(got - ref) - allow, 0.0)
    assert np.isfinite(over).all()
    assert (over[scale == 0] == 0).all()
    return float((over[scale > 0] / scale[scale > 0]).max(initial=0.0))


def row_err(got, ref, top=None):
    """row-wise: max_j |got - ref| / top per row (top: the row's scale, max_j |ref| by default), the worst row; a row whose
    scale is 0 must be all 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max(1) if top is None else np.asarray(top, np.float64)
    d = np.abs(got - ref).max(1)
    assert np.isfinite(d).all()
    assert (d[top == 0] == 0).all()
    return float((d[top > 0] / top[top > 0]).max(initial=0.0))


# ---- the input families ---------------------------------------------------------------------------------------------------------
def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def mask_of(kind, n=HEAD_N, begin=HEAD_BEGIN, end=HEAD_END):
    if kind == "none":
        return None
    m = np.zeros(n, np.uint8)
    if kind == "third":
        m[begin:end:3] = 1
    elif kind == "ones":
        m[:] = 1
    elif kind == "two":  # 0, 1 and 2 in turn: the byte 2 is "out"
        m[:] = np.arange(n) % 3
    else:
        assert kind == "zeros"
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def softmax_family(name, C, n=HEAD_N):
    """(logits [n][C] fp32, labels [n] bytes below C), read-only"""
    rng = np.random.default_rng([_seed(name), C, n])
    lab = rng.integers(0, C, n)
    x = (3.0 * rng.standard_normal((n, C))).astype(np.float32)
    r = np.arange(n)
    if name == "offset":
        x = (x + rng.choice(np.float32([-3e4, 3e4]), n)[:, None]).astype(np.float32)
    elif name == "wide":  # the maximum 0 in one place, -80 in another, a quarter of the rest 110 to 150 below, the others within 80
        x = -rng.uniform(0.0, 80.0, (n, C))
        low = rng.random((n, C)) < 0.25
        x[low] = -rng.uniform(110.0, 150.0, int(low.sum()))
        top = rng.integers(0, C, n)
        x[r, top] = 0.0
        if C > 1:
            x[r, (top + 1 + rng.integers(0, C - 1, n)) % C] = -80.0
        x = x.astype(np.float32)
    elif name == "clamp":  # the label's logit 110.5 to 140 below the maximum of the others (C = 1: no such row exists)
        if C > 1:
            x[r, lab] = -np.inf
            x[r, lab] = x.max(1) - rng.uniform(110.5, 140.0, n).astype(np.float32)
    elif name == "ties":  # integers; row 4k: all equal; row 4k + 1: the maximum two or three times, not first in the row
        x = rng.integers(-3, 4, (n, C)).astype(np.float32)
        x[0::4] = x[0::4, :1]
        for i in range(1, n, 4):
            x[i, rng.integers(0, C, 3)] = 5.0
    elif name == "spike":  # one logit at 1e4, the rest 0; every other label is the spike
        x = np.zeros((n, C), np.float32)
        at = rng.integers(0, C, n)
        x[r, at] = 1e4
        lab[0::2] = at[0::2]
    else:
        assert name == "benign"
    xm = x.astype(np.float64) - x.astype(np.float64).max(1, keepdims=True)
    gap = xm[r, lab]
    assert ((gap >= -80.0) | (gap <= -110.0)).all(), name  # never the band where fp32 expf is subnormal or flushed
    if name == "wide":
        assert xm.min() <= -110 or C <= 2  # (two classes hold the 0 and the -80 alone)
        assert C == 1 or (xm == -80.0).any(1).all()
    if name == "clamp" and C > 1:
        assert (gap <= -110.0).all()
    lab = lab.astype(np.uint8)
    x.setflags(write=False)
    lab.setflags(write=False)
    return x, lab


SIG_KNOWN = ((0, np.float32(0.0)), (1, np.float32(-0.0)), (2, np.float32(88.8)), (3, np.float32(-88.8)))  # (row - begin, value)


@functools.lru_cache(maxsize=None)
def sigmoid_family(name, C, n=HEAD_N, begin=HEAD_BEGIN):
    """(logits [n][C] fp32, labels [n][C] bytes 0 / 1); rows begin .. begin + 3 hold 0.0, -0.0, 88.8, -88.8 in their first and
    last column"""
    rng = np.random.default_rng([_seed(name) + 1, C, n])
    y = (rng.random((n, C)) < 0.3).astype(np.uint8)
    x = rng.standard_normal((n, C))
    if name == "benign":
        x = 3.0 * x
    elif name == "offset":
        x = 3.0 * x + rng.choice([-3e4, 3e4], n)[:, None]
    elif name == "wide":
        x = rng.uniform(-80.0, 80.0, (n, C))
    elif name == "ties":
        x = rng.integers(-3, 4, (n, C)).astype(np.float64)
    elif name == "spike":
        x = np.zeros((n, C))
        x[np.arange(n), rng.integers(0, C, n)] = 1e4
    elif name == "scale100":
        x = 100.0 * x
    else:
        assert name == "scale1e4"
        x = 1e4 * x
    x = x.astype(np.float32)
    for k, v in SIG_KNOWN:
        x[begin + k, 0] = x[begin + k, C - 1] = v
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def l2_family(n, dim):
    """(x, g, kind [n]): row i is of family L2_FAMILIES[i % 4] -- benign, exactly 0, 1e-8 (the clamp is active up to dim 1000:
    1000 x 1e-16 < 1e-12), 1e15 (the sum of squares, at most 1e33, is finite)"""
    rng = np.random.default_rng([77, n, dim])
    x = rng.standard_normal((n, dim))
    kind = np.arange(n) % 4
    x[kind == 1] = 0.0
    x[kind == 2] = 1e-8 * np.sign(x[kind == 2])
    x[kind == 3] = 1e15 * np.sign(x[kind == 3])
    x, g = x.astype(np.float32), rng.standard_normal((n, dim)).astype(np.float32)
    assert ((x[kind == 2].astype(np.float64) ** 2).sum(1) < 1e-12).all()
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g, kind


@functools.lru_cache(maxsize=None)
def adam_grad(name, n, seed=0):
    """N(0,1); +-(1e-6 .. 1e-4); exactly 0; +-1e18; the four mixed element by element"""
    rng = np.random.default_rng([91, _seed(name), n, seed])
    normal = rng.standard_normal(n)
    small = rng.uniform(1e-6, 1e-4, n) * rng.choice([-1.0, 1.0], n)  # g^2 from 1e-12 to 1e-8: eps = 1e-8 decides the step
    pick = {"normal": normal, "small": small, "zero": np.zeros(n), "huge": np.full(n, 1e18) * rng.choice([-1.0, 1.0], n)}
    if name == "mixed":
        which = rng.integers(0, 4, n)
        g = np.choose(which, [pick[k] for k in ("normal", "small", "zero", "huge")])
    else:
        g = pick[name]
    g = g.astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def adam_state(name, n):
    """(W, m, v) fp32: all zero moments, or the moments three fp64 steps of N(0,1) gradients leave (rounded to fp32)"""
    rng = np.random.default_rng([92, n])
    W = rng.standard_normal(n).astype(np.float32)
    m, v = np.zeros(n), np.zeros(n)
    if name == "warm":
        for s in range(3):
            g = adam_grad("normal", n, seed=100 + s).astype(np.float64)
            m, v = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
    out = (W, m.astype(np.float32), v.astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


def relu_data(n):
    """NaN, +-0, +-inf, the subnormals and the ordinary, in turn"""
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39, 1.5, -1.5, 3e38, -3e38], np.float32)
    rng = np.random.default_rng([93, n])
    x = rng.standard_normal(n).astype(np.float32)
    k = min(n, 4 * len(special))
    x[:k] = special[(np.arange(k) + n) % len(special)]
    g = rng.standard_normal(n).astype(np.float32)
    g[:k] = special[(np.arange(k) * 5 + 1) % len(special)]
    return x, g


def tie_preds(n, C, seed=0):
    """predictions with ties for the accuracy: the softmax `ties` rows, then by row % 8: 5 -> all -inf, 6 -> all NaN,
    7 -> NaN in the first place and behind the maximum; labels: the first maximum, the second one, or any class"""
    rng = np.random.default_rng([94, n, C, seed])
    x = rng.integers(-3, 4, (n, C)).astype(np.float32)
    x[0::4] = x[0::4, :1]
    r = np.arange(1, n, 4)
    x[r[:, None], rng.integers(0, C, (len(r), 3))] = 5.0
    lab = rng.integers(0, C, n)
    lab[0::3] = x.argmax(1)[0::3]
    lab[1::3] = (C - 1 - x[:, ::-1].argmax(1))[1::3]  # the LAST maximum: a hit only where the maximum is single
    x[5::8] = -np.inf
    x[6::8] = np.nan
    x[7::8, 0] = np.nan
    if C > 2:
        x[7::8, C - 1] = np.nan
    return x, lab.astype(np.uint8)
