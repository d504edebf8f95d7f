"""GPU suite: non-finite values in an operand of a dense product reach only the rows / columns of C that depend on them
(tests/poison.py has the method).  Every kernel form behind gaib_sgemm_ex, gaib_sgemm_drelu and gaib_gemm_bf16 at the smallest
shape the dispatch sends to it (poison.DENSE_FORMS names the sgemm_variant where a form has to be forced):

  * M side: +inf in every odd row of the M-side operand (rows of A; columns of A for TN): even rows of C keep the clean run's
    bits, odd rows are not finite.  For a row-major A this also catches a K tail read over into the next row against a
    zero-padded B.  N side: the same with every odd column of the N-side operand.
  * K edges: both operands positive, +inf at k = 0 -- the row the kernels point idle K steps at -- and at the last four k of
    the odd rows (columns) only: the dependent entries are +inf EXACTLY.  A dummy row or a K tail multiplied against a zeroed
    partner instead of being selected away shows as NaN in a dependent entry (0 * inf), which the two cases above accept.
    (gaib_sgemm_ex only: an fp32 product, where Inf times a positive number is +inf.)
  * with accum, +inf at a few entries of C0: those entries are +inf, nothing else moves.  Without accum C is pre-filled with NaN
    bits and nothing of them may survive; the 64 elements behind C never change.  relu on and off.
  * gaib_sgemm_drelu: +inf and NaN in G exactly where mask <= 0, NaN at a few mask entries: G comes back with +0.0 bits there
    and its own bits elsewhere, C keeps the clean run's bits -- through all the kernels that take the mask (sgemm_variant 0, 30, 34).

Operands are views into larger allocations between NaN guard elements; the clean run is held to A.double() @ B.double() on the
device (LONG_SUM_FLOOR from K = 1024 on, as util.py says)."""
import numpy as np
import pytest
import torch

import poison as P
from util import LONG_SUM_FLOOR, ELEM_FLOOR, assert_close_dev

pytestmark = pytest.mark.gpu

INF = float("inf")
C0_POISON = ((0, 0), (1, 2), (-1, -1), (-2, 0), (7, -3))


@pytest.fixture
def variant(ctx):
    """sets sgemm_variant for one test, then back to the dispatch's own rule"""
    try:
        yield lambda v: ctx.set_option("sgemm_variant", v)
    finally:
        ctx.set_option("sgemm_variant", 0)


def guarded(shape, seed, dtype=torch.float32):
    """N(0,1) on the device, a view into a larger allocation with P.GUARD NaN elements either side -> (buffer, view)"""
    n = int(np.prod(shape))
    buf = P.nan_fill(torch.empty(n + 2 * P.GUARD, dtype=dtype, device="cuda"))
    view = buf[P.GUARD:P.GUARD + n].view(*shape)
    view.copy_(torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)))
    return buf, view


def with_poison(buf, shape, write):
    """a copy of a guarded operand (guards included) with write(view) applied"""
    b = buf.clone()
    v = b[P.GUARD:P.GUARD + int(np.prod(shape))].view(*shape)
    write(v)
    return v


def bits(t):
    return t.contiguous().view(torch.int32)


def result(out, what):
    """C of a P.Out on the device: the tail untouched, nothing of the pre-fill left"""
    n = out.t.numel()
    assert bool((bits(out.buf[n:]) == P.NAN_BITS).all()), f"{what}: the elements past the end of C were written"
    assert not bool((bits(out.t) == P.NAN_BITS).any()), f"{what}: C left unwritten"
    return out.t


def compare(clean, dirty, dep, cls, what):
    """P.compare on the device (C has up to 65537 x 128 entries)"""
    assert bool(torch.isfinite(clean).all()), f"{what}: the clean run is not finite"
    diff = (bits(clean) != bits(dirty)) & ~dep
    if bool(diff.any()):
        i = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} independent entries changed with the poison, first at {i}: "
                             f"{clean[i].item()!r} -> {dirty[i].item()!r}")
    v = dirty[dep]
    bad = {"+inf": ~torch.isposinf(v), "nonfinite": torch.isfinite(v), "+inf|0": ~(torch.isposinf(v) | (v == 0))}[cls]
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {v.numel()} dependent entries are not {cls}, first {v[bad][0].item()!r}"


def odd(view, axis):
    if axis == 0:
        view[1::2] = INF
    else:
        view[:, 1::2] = INF


def k_edges(view, k_axis, K):
    """+inf at k = 0 and the last four k of every odd row / column of the other axis"""
    ks = [0] + list(range(max(K - 4, 1), K))
    if k_axis == 0:
        view[ks, 1::2] = INF
    else:
        for k in ks:
            view[1::2, k] = INF


def positive(buf, shape):
    return with_poison(buf, shape, lambda v: v.copy_(v.abs() + 0.1))


@pytest.mark.parametrize("form,tA,tB,M,N,K,sv", P.DENSE_FORMS, ids=[f"{f[0].replace(' ', '_')}-{f[3]}x{f[4]}x{f[5]}" for f in P.DENSE_FORMS])
def test_sgemm(ctx, variant, form, tA, tB, M, N, K, sv):
    variant(sv)
    sa, sb = ((K, M) if tA else (M, K)), ((N, K) if tB else (K, N))
    abuf, A = guarded(sa, 1000 + M)
    bbuf, B = guarded(sb, 2000 + N)
    _, C0 = guarded((M, N), 3000 + K)
    ref = (A.double().t() if tA else A.double()) @ (B.double().t() if tB else B.double())
    floor = LONG_SUM_FLOOR if K >= 1024 else ELEM_FLOOR
    Ap = with_poison(abuf, sa, lambda v: odd(v, 1 if tA else 0))   # odd rows of op(A)
    Bp = with_poison(bbuf, sb, lambda v: odd(v, 0 if tB else 1))   # odd columns of op(B)
    deps = {s: torch.from_numpy(P.dense_dependent(M, N, s)).cuda() for s in "MN"}
    for s in "MN":
        P.shares(P.dense_dependent(M, N, s), f"{form} {s}")

    def run_as(accum, relu, what):
        def run(a, b, c0, tag):
            out = P.Out(M, N)
            if accum:
                out.t.copy_(c0)
            ctx.sgemm(a, b, out.t, transA=bool(tA), transB=bool(tB), accum=accum, relu=relu)
            return result(out, f"{what} {tag}")
        return run

    for accum, relu in ((False, False), (False, True), (True, False)):
        what = f"{form} {M} x {N} x {K} variant {sv} accum {accum} relu {relu}"
        run = run_as(accum, relu, what)
        clean = run(A, B, C0, "clean")
        want = ref + C0.double() if accum else ref
        assert_close_dev(clean, want.clamp_min(0) if relu else want, what, floor=floor)
        cls = "+inf|0" if relu else "nonfinite"
        compare(clean, run(Ap, B, C0, "M side"), deps["M"], cls, what + " M side")
        compare(clean, run(A, Bp, C0, "N side"), deps["N"], cls, what + " N side")
        if accum:
            C0p = C0.clone()
            dep = torch.zeros(M, N, dtype=torch.bool, device="cuda")
            for i, j in C0_POISON:
                C0p[i, j] = INF
                dep[i, j] = True
            compare(clean, run(A, B, C0p, "C0"), dep, "+inf", what + " C0")
    # K edges on positive operands: exactly +inf
    apos, bpos = positive(abuf, sa), positive(bbuf, sb)
    Ae = with_poison(abuf, sa, lambda v: (v.copy_(v.abs() + 0.1), k_edges(v, 0 if tA else 1, K)))
    Be = with_poison(bbuf, sb, lambda v: (v.copy_(v.abs() + 0.1), k_edges(v, 1 if tB else 0, K)))
    for relu in (False, True):
        what = f"{form} {M} x {N} x {K} variant {sv} positive operands relu {relu}"
        run = run_as(False, relu, what)
        clean = run(apos, bpos, None, "clean")
        assert_close_dev(clean, (apos.double().t() if tA else apos.double()) @ (bpos.double().t() if tB else bpos.double()), what, floor=floor)
        compare(clean, run(Ae, bpos, None, "M side K edges"), deps["M"], "+inf", what + " M side K edges")
        compare(clean, run(apos, Be, None, "N side K edges"), deps["N"], "+inf", what + " N side K edges")


# (M, N, K, the sgemm_variants that send it to each kernel taking the mask)
DRELU = [(128, 128, 32769, {0: "register-resident", 30: "LDS-tiled"}),
         (256, 256, 32769, {0: "LDS ring", 34: "register teams", 30: "LDS-tiled"}),
         (132, 196, 4097, {0: "LDS-tiled, split K"}),
         (100, 128, 65537, {0: "wide tn, seven tiles", 30: "LDS-tiled"})]


@pytest.mark.parametrize("M,N,K,variants", DRELU, ids=[f"{m}x{n}x{k}" for m, n, k, _ in DRELU])
@pytest.mark.parametrize("accum", [False, True])
def test_sgemm_drelu(ctx, variant, M, N, K, variants, accum):
    """G <- G where mask > 0 else +0.0 (in place), C (+)= A^T . G"""
    _, A = guarded((K, M), 4000 + M)
    gbuf, G = guarded((K, N), 5000 + N)
    mbuf, mask = guarded((K, N), 6000 + K)
    _, C0 = guarded((M, N), 7000)
    mask[torch.rand(K, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(K)) < 0.1] = 0.0  # exact zeros are out too
    off = mask <= 0
    nan_at = [(0, 0), (K - 1, N - 1), (K // 2, 1), (K - 1, 0), (5, N - 2)]
    for i, j in nan_at:            # the clean run has a 0 where the poisoned mask has a NaN: masked either way
        mask[i, j] = 0.0
        off[i, j] = True
    assert 0.4 < off.float().mean().item() < 0.7

    def put(v):
        v[off] = INF
        v[off & (torch.arange(N, device="cuda")[None, :] % 3 == 0)] = float("nan")

    Gp = with_poison(gbuf, (K, N), put)

    def put_mask(v):
        for i, j in nan_at:
            v[i, j] = float("nan")

    maskp = with_poison(mbuf, (K, N), put_mask)
    gm = torch.where(off, torch.zeros_like(G), G)
    ref = A.double().t() @ gm.double() + (C0.double() if accum else 0)
    for sv, name in variants.items():
        variant(sv)
        what = f"sgemm_drelu {M} x {N} x {K} variant {sv} ({name}) accum {accum}"

        def run(g_in, m_in, tag):
            out = P.Out(M, N)
            if accum:
                out.t.copy_(C0)
            buf = P.nan_fill(torch.empty(K * N + 2 * P.GUARD, device="cuda"))
            g = buf[P.GUARD:P.GUARD + K * N].view(K, N)
            g.copy_(g_in)
            ctx.sgemm_drelu(A, g, m_in, out.t, accum=accum)
            ctx.sync()
            assert bool((bits(buf[:P.GUARD]) == P.NAN_BITS).all() and (bits(buf[-P.GUARD:]) == P.NAN_BITS).all()), f"{what} {tag}: G's guards written"
            return result(out, f"{what} {tag}"), g

        c_clean, g_clean = run(G, mask, "clean")
        assert_close_dev(c_clean, ref, what, floor=LONG_SUM_FLOOR)
        assert torch.equal(bits(g_clean), bits(gm)), what + ": G"
        c_dirty, g_dirty = run(Gp, maskp, "poisoned")
        assert torch.equal(bits(g_dirty), bits(gm)), what + ": G is not +0.0 bits where mask <= 0 (or NaN) and its own bits elsewhere"
        assert (g_dirty[off].view(torch.int32) == 0).all()
        assert torch.equal(bits(c_clean), bits(c_dirty)), what + ": C changed with what lies under the mask"


GEMM_BF16 = [(65, 24, 36, 32), (65, 40, 100, 40), (33, 72, 132, 80), (65, 136, 256, 136), (257, 256, 64, 264)]  # (M, K, N, lda)


@pytest.mark.parametrize("M,K,N,lda", GEMM_BF16, ids=[f"{m}x{k}x{n}" for m, k, n, _ in GEMM_BF16])
@pytest.mark.parametrize("transB", [False, True])
def test_gemm_bf16(ctx, M, K, N, lda, transB):
    """the bf16 table's product at each of its four K depths (k-steps of 32: K <= 32, 64, 128, 256), one K that is no whole
    step each, pad columns behind K holding NaN.  No K-edge case here: the product is defined over B split into three bf16
    planes whose second and third carry either sign (and are 0 - inf = NaN for an Inf in B), so an Inf operand gives "not
    finite" by definition, never exactly +inf"""
    assert ctx.gemm_bf16_cover(N, K, lda, transB)
    abuf, A = guarded((M, lda), 8000 + M, torch.bfloat16)
    A[:, K:] = float("nan")
    sb = (N, K) if transB else (K, N)
    bbuf, B = guarded(sb, 8100 + N)
    _, C0 = guarded((M, N), 8200)
    ref = A[:, :K].double() @ (B.double().t() if transB else B.double())
    Ap = with_poison(abuf, (M, lda), lambda v: v[1::2, :K].fill_(INF))
    Bp = with_poison(bbuf, sb, lambda v: odd(v, 0 if transB else 1))
    deps = {s: torch.from_numpy(P.dense_dependent(M, N, s)).cuda() for s in "MN"}
    for s in "MN":
        P.shares(P.dense_dependent(M, N, s), f"gemm_bf16 {M} x {N} x {K} {s}")
    for accum, relu in ((False, False), (False, True), (True, False)):
        what = f"gemm_bf16 {M} x {N} x {K} lda {lda} transB {transB} accum {accum} relu {relu}"

        def run(a, b, c0, tag):
            out = P.Out(M, N)
            if accum:
                out.t.copy_(c0)
            ctx.gemm_bf16(a, b, out.t, K=K, transB=transB, accum=accum, relu=relu)
            return result(out, f"{what} {tag}")

        clean = run(A, B, C0, "clean")
        want = ref + C0.double() if accum else ref
        assert_close_dev(clean, want.clamp_min(0) if relu else want, what)
        cls = "+inf|0" if relu else "nonfinite"
        compare(clean, run(Ap, B, C0, "M side"), deps["M"], cls, what + " M side")
        compare(clean, run(A, Bp, C0, "N side"), deps["N"], cls, what + " N side")
        if accum:
            C0p = C0.clone()
            dep = torch.zeros(M, N, dtype=torch.bool, device="cuda")
            for i, j in C0_POISON:
                C0p[i, j] = INF
                dep[i, j] = True
            compare(clean, run(A, B, C0p, "C0"), dep, "+inf", what + " C0")
