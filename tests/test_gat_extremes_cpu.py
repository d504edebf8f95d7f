"""The inputs of the extreme-score GAT tests (tests/gat_ref64.py) and the fp32 oracle on them, without a GPU: every family
keeps what it promises (the asserts of gat_ref64.check_family and of the two graphs), the oracle stays finite, and the oracle
alone stays within the bounds the GPU tests (tests/test_gpu_gat_extremes.py) give the kernels -- assert_close's default for
out, the attention and grad_out, 2^-23 of the summed magnitude for the alpha gradients.  On `underflow` (score ranges past
100, where an fp32 softmax keeps one term of a row) the oracle's distance is printed, not bounded.

Measured (oracle against fp64, the worst over the three shapes) -- out / attention / grad_out element-wise, alpha in units of
scale_l / scale_r:
    wide 5.7e-5 / 6.3e-6 / 1.1e-5 / 2.7e-8    asc 2.1e-5 / 1.4e-5 / 4.3e-5 / 4.5e-9    desc 1.8e-5 / 1.4e-5 / 3.4e-5 / 1.0e-8
    uniform 1.5e-6 / 4.5e-8 / 8.5e-6 / 1.7e-8    zero 1.6e-6 / 4.5e-8 / 8.7e-6 / 2.6e-8    benign 1.1e-5 / 8.7e-7 / 5.7e-6 / 1.5e-8
    underflow 3.5e-4 / 1.8e-5 / 8.9e-5 / 3.1e-8  (its alpha gradients are bounded like the others')"""
import numpy as np
import pytest

import gat_ref64 as R
from util import assert_close, elem_err

ALPHA_CAP = 2.0 ** -23  # of scale_l / scale_r


def test_the_graphs():
    rp, ci = R.graph_a()
    deg = np.diff(rp)
    assert len(rp) - 1 == 400 and deg[R.HUB] == 4 * 64 + 45 and (deg == 64).any() and (deg == 65).any() and (deg == 1).any()
    assert all(i in ci[rp[i]:rp[i + 1]] for i in range(len(deg)))  # self loops
    rp, ci = R.graph_b()
    deg = np.diff(rp)
    assert (deg == 0).sum() >= 10 and (deg == 1).sum() >= 10
    assert not any(i in ci[rp[i]:rp[i + 1]] for i in range(len(deg)))  # none


def test_reference_against_a_dense_evaluation():
    """gat_ref64 against the same formulas written with dense matrices and autograd-free calculus on 12 vertices: the
    alpha gradients are the derivatives of <out, grad> by finite differences in fp64"""
    rng = np.random.default_rng(3)
    n, d, heads = 12, 8, 2
    A = rng.random((n, n)) < 0.4
    A = A | A.T
    A[5] = A[:, 5] = False  # a row without an edge
    rp = np.concatenate([[0], np.cumsum(A.sum(1))]).astype(np.int64)
    ci = np.nonzero(A)[1].astype(np.uint32)
    h, g = rng.standard_normal((n, d)), rng.standard_normal((n, d))
    al, ar = rng.standard_normal(d), rng.standard_normal(d)
    mask = (rng.random((len(ci), heads)) < 0.6).astype(np.float64)
    for m, sc in ((None, 1.0), (mask, 1.7)):
        ref = R.reference(rp, ci, h, al, ar, g, heads, mask=m, scale=sc)
        loss = lambda a_l, a_r: (R.gat_ref64(rp, ci, h, a_l, a_r, g, heads, mask=m, scale=sc)[2] * g).sum()
        step = 1e-6
        for j in range(d):
            e = np.zeros(d)
            e[j] = step
            assert abs((loss(al + e, ar) - loss(al - e, ar)) / (2 * step) - ref.lg[j]) <= 1e-7 * max(1, abs(ref.lg[j]))
            assert abs((loss(al, ar + e) - loss(al, ar - e)) / (2 * step) - ref.rg[j]) <= 1e-7 * max(1, abs(ref.rg[j]))
        # out and grad_out are the two sides of one bilinear form: <out(h'), g> = <h', grad_out> for a gathered table h'
        assert (ref.out[5] == 0).all() and (ref.grad_out[5] == 0).all()
        P = np.zeros((heads, n, n))
        P[:, R.rows_of(rp), ci.astype(np.int64)] = (ref.p * (1 if m is None else m * sc)).T
        dh = d // heads
        for k in range(heads):
            sl = slice(k * dh, (k + 1) * dh)
            assert np.allclose(P[k] @ h[:, sl], ref.out[:, sl], rtol=1e-12, atol=1e-14)
            assert np.allclose(P[k].T @ g[:, sl], ref.grad_out[:, sl], rtol=1e-12, atol=1e-14)
        assert np.allclose(ref.p.sum(0), (np.diff(rp) > 0).sum())  # every row with an edge sums to 1


@pytest.mark.parametrize("d,heads", R.SHAPES)
@pytest.mark.parametrize("name", R.FAMILIES)
def test_family_and_oracle(name, d, heads):
    rp, ci, h, al, ar, grad = R.family(name, d, heads)  # (asserts what the family promises)
    ref, orc_ = R.family_reference(name, d, heads)
    for key in ("out", "temp", "p", "grad_out", "lg", "rg"):
        assert np.isfinite(getattr(orc_, key)).all(), key
    for key in ("t", "p", "out", "grad_out", "lg", "rg", "scale_l", "scale_r"):
        assert np.isfinite(getattr(ref, key)).all(), key
    deg = np.diff(rp)
    if name in ("uniform", "zero"):
        assert np.allclose(ref.p, (1.0 / deg)[R.rows_of(rp)][:, None], rtol=1e-12, atol=0)
        # one slope per row and sum_e ds_e = 0: the true alpha_l gradient is 0 (the column sums, and so alpha_r's, are not)
        assert R.alpha_ratio(ref.lg, 0, ref.scale_l) < 1e-12
    ra = max(R.alpha_ratio(orc_.lg, ref.lg, ref.scale_l), R.alpha_ratio(orc_.rg, ref.rg, ref.scale_r))
    errs = {k: elem_err(getattr(orc_, k), getattr(ref, k)) for k in ("out", "p", "grad_out")}
    print(f"{name} {d}x{heads}: oracle against fp64: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" alpha {ra:.2e} of the scale")
    assert ra <= ALPHA_CAP, ra
    if name != "underflow":
        for k in errs:
            assert_close(getattr(orc_, k), getattr(ref, k), f"{name} {d}x{heads} oracle {k}")
