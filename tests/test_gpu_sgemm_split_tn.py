"""GPU suite, gaib_sgemm_split_tn: the fp32 weight gradient C (=|+=) A^T . G on the bf16 matrix cores with both operands split
exactly into three bf16 planes, plain and with gaib_sgemm_drelu's mask.  Exact cases (integer sums that need the cross planes; one
full-range term per output), the derived bound on random data and bit identity of two runs, the refusals and the switch
sgemm_split_tn of gaib_sgemm_ex / gaib_sgemm_drelu, the GCN / SAGE layers and the trainer under the option."""
import os
import re
import subprocess
from functools import lru_cache
from math import gcd
from pathlib import Path

import pytest
import torch

import layer_ref64 as LR
from test_gpu_bf16 import make_dataset
from test_gpu_layers_exact import graphs, layer, lctx  # noqa: F401  (fixtures of the exact layer cells)

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
U32 = 2.0 ** -23
GUARD = 64  # floats of NaN bits in front of and behind A, G and C (256 bytes: the arrays stay on 16-byte boundaries)
SHAPES = [(1, 4, 4), (31, 16, 16), (33, 100, 128), (257, 128, 128), (300, 256, 256), "grid"]  # (K, M, N)
IDS = ["x".join(map(str, s)) if s != "grid" else s for s in SHAPES]


def resolve(ctx, shape):
    """a basic shape as it is; "grid": M = N = 256 and the smallest K at which every workgroup of a full grid runs its steady loop,
    the counts differ and the last k-step is partial.  The launcher's grid rule (sgemm_split_tn.hip, split_tn_parts): k-steps of 32
    rows, P = min(num_cus / 2 column slabs, k-steps / 4) workgroups per slab, workgroup b takes the k-steps b, b + P, ...  With
    4 P + P / 2 k-steps P is at its cap, the first half of the workgroups has 5 k-steps, the second 4; K = 32 k-steps - 5."""
    if shape != "grid":
        return shape
    P = ctx.get_option("num_cus") // 2
    steps = 4 * P + P // 2
    K = 32 * steps - 5
    assert ctx.sgemm_split_tn_parts(256, 256, K) == P > 1 and K % 32 != 0
    assert {(steps - b + P - 1) // P for b in range(P)} == {4, 5}
    return (K, 256, 256)


def bits32(t):
    return t.contiguous().view(torch.int32)


def run(ctx, a, g, mask=None, C0=None):
    """gaib_sgemm_split_tn on A [K x M], G [K x N] (and mask), each between guard bands of NaN bits: a NaN in the result means a
    band was consumed.  Returns C and G as the call left them, on the host."""
    (K, M), N = a.shape, g.shape[1]

    rawA, rawG, rawC = (torch.full((2 * GUARD + n,), float("nan")) for n in (K * M, K * N, M * N))
    for raw, t in ((rawA, a), (rawG, g), (rawC, C0)):
        if t is not None:
            raw[GUARD:GUARD + t.numel()] = t.reshape(-1)
    rawA, rawG, rawC = rawA.cuda(), rawG.cuda(), rawC.cuda()
    Am, Gm, Cm = rawA[GUARD:GUARD + K * M].view(K, M), rawG[GUARD:GUARD + K * N].view(K, N), rawC[GUARD:GUARD + M * N].view(M, N)
    ctx.sgemm_split_tn(Am, Gm, Cm, mask=None if mask is None else mask.cuda(), accum=C0 is not None)
    torch.cuda.synchronize()
    for raw, n in ((rawG, K * N), (rawC, M * N)):
        assert bool(torch.isnan(raw[:GUARD]).all()) and bool(torch.isnan(raw[GUARD + n:]).all()), "a guard band was written"
    return Cm.cpu(), Gm.cpu()


@lru_cache(maxsize=None)
def int_case(kind, K, M, N):
    """a: 21-bit odd entries in A, three per column and spread over all of K, against G = +-1 (A's third plane); b: the mirror
    image; c: 11-bit odd entries, three per column of A, against a dense odd 11-bit G (plane 1 x plane 1)"""
    gen = torch.Generator().manual_seed(7 * K + M + N)
    bits_a, bits_g = {"a": (21, 1), "b": (1, 21), "c": (11, 11)}[kind]

    def odd(shape, bits):
        mag = torch.randint(1 << (bits - 2), 1 << (bits - 1), shape, generator=gen) * 2 + 1 if bits > 1 else torch.ones(shape, dtype=torch.int64)
        return (mag * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()

    def sparse(W, bits):
        t = torch.zeros(K, W)
        c = torch.arange(W)
        for rows in (c * (K // W + 1), K - 1 - c, 7 * c + 3):
            t[rows % K, c] = odd((W,), bits)
        return t

    a = odd((K, M), bits_a) if kind == "b" else sparse(M, bits_a)
    g = sparse(N, bits_g) if kind == "b" else odd((K, N), bits_g)
    c0 = torch.randint(-(1 << 20) + 1, 1 << 20, (M, N), generator=gen).float()
    mask = torch.randint(-1, 2, (K, N), generator=gen).float()
    poison = torch.tensor([float("nan"), float("inf"), float("-inf")])[torch.randint(0, 3, g.shape, generator=gen)]
    g_in, g_out = torch.where(mask > 0, g, poison), torch.where(mask > 0, g, torch.zeros(()))  # before the call, after it
    assert float((a.double().abs().T @ g.double().abs() + c0.double().abs()).max()) < 2 ** 24  # every partial sum is exact
    return a, g, c0, mask, g_in, g_out, a.double().T @ g.double(), a.double().T @ g_out.double()


@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_integer_sums_are_exact(ctx, shape, masked, accum):
    K, M, N = resolve(ctx, shape)
    for kind in "abc":
        a, g, c0, mask, g_in, g_out, plain, under_mask = int_case(kind, K, M, N)
        want = (under_mask if masked else plain) + (c0.double() if accum else 0)
        got, g_after = run(ctx, a, g_in if masked else g, mask if masked else None, c0 if accum else None)
        assert not torch.isnan(got).any(), (kind, shape, "a NaN in C: a guard band or a masked-out element was consumed")
        bad = got.double() != want
        assert not bad.any(), (kind, shape, masked, accum, int(bad.sum()), got[bad][:4], want[bad][:4])
        assert torch.equal(bits32(g_after), bits32(g_out if masked else g)), (kind, shape, masked)


@lru_cache(maxsize=None)
def one_term(K, M, N):
    """term i < min(M, K) sits in row (i stride) % K (stride co-prime to K: distinct rows all over K), column i of A, at exponent
    -90, 0 or 126.  Even i: A holds all 24 mantissa bits and the row of G is +-2^e; odd i: A is +-2^e and the row of G holds full
    mantissas (lowest bit set) times 2^e -- each product has 24 bits"""
    gen = torch.Generator().manual_seed(100 + K)
    stride = next(s for s in range(max(1, K // M), 2 * K + 2) if gcd(s, K) == 1)
    i = torch.arange(min(M, K))
    rows = (i * stride) % K
    assert len(set(rows.tolist())) == len(i)
    sgn = torch.randint(0, 2, i.shape, generator=gen).double() * 2 - 1
    mant = torch.where(i % 2 == 0, torch.tensor(2.0 - 2.0 ** -23, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    a = torch.zeros(K, M)
    a[rows, i] = (sgn * mant * torch.exp2(torch.tensor([-90.0, 0.0, 126.0], dtype=torch.float64)[i % 3])).float()
    full = ((torch.randint(0, 1 << 23, (K, N), generator=gen) | 1) + (1 << 23)).double() * 2.0 ** -23  # [1, 2), 24 bits
    scale = torch.exp2(torch.randint(-20, 1, (K, N), generator=gen).double()) * (torch.randint(0, 2, (K, N), generator=gen) * 2 - 1)
    even = torch.ones(K, dtype=torch.bool)
    even[rows] = i % 2 == 0
    g = (torch.where(even[:, None], torch.ones(K, N, dtype=torch.float64), full) * scale).float()
    want = a.double().T @ g.double()
    assert bool(torch.isfinite(want).all()) and torch.equal(want.float().double(), want)  # the fp64 product is an fp32 value
    return a, g, want.float()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_term_per_output_is_exact(ctx, shape):
    a, g, want = one_term(*resolve(ctx, shape))
    got, _ = run(ctx, a, g)
    assert not torch.isnan(got).any()
    bad = bits32(got + 0.0) != bits32(want + 0.0)  # (+ 0.0: an output without a term is a zero of either sign)
    assert not bad.any(), (shape, int(bad.sum()), got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_data_within_the_bound(ctx, shape, masked, accum):
    """The truncated planes of a value have its sign and sum to it exactly, so the nine plane products of a term are exact, have
    one sign and sum to |a| |g'|: an output is a sum of 9 K exact terms in the accumulators of the workgroups, then `parts`
    partial sums and the old C in the reduction -- at most 9 K + parts + 1 additions, one ulp of the running sum (at most 2^-23,
    whether an addition inside the matrix core rounds or truncates) each, and every running sum is at most the sum of the
    magnitudes: |C - C64| <= (9 K + parts + 2) 2^-23 (|A|^T |G'| + |C0|), the + 1 covering the second-order terms."""
    K, M, N = resolve(ctx, shape)
    gen = torch.Generator().manual_seed(K + M)
    a, g = torch.randn(K, M, generator=gen), torch.randn(K, N, generator=gen)
    mask = torch.sign(torch.randn(K, N, generator=gen)) if masked else None
    gm = torch.where(mask > 0, g, torch.zeros(())) if masked else g
    c0 = torch.randn(M, N, generator=gen) if accum else None
    got, g_after = run(ctx, a, g, mask, c0)
    assert torch.equal(bits32(g_after), bits32(gm))
    c64 = a.double().T @ gm.double() + (c0.double() if accum else 0)
    parts = ctx.sgemm_split_tn_parts(M, N, K)
    bound = (9 * K + parts + 2) * U32 * (a.double().abs().T @ gm.double().abs() + (c0.double().abs() if accum else 0))
    err = (got.double() - c64).abs()
    print(f"{shape} masked={masked} accum={accum} parts={parts}: worst err / bound = {float((err / bound.clamp(min=1e-300)).max()):.5f}")
    assert bool((err <= bound).all()), (shape, masked, accum, float((err - bound).max()))
    assert torch.equal(bits32(run(ctx, a, g, mask, c0)[0]), bits32(got))  # the same call twice: the same bits


def test_refusals_leave_c_and_g_untouched(ctx):
    lib, h = ctx.lib, ctx.h
    K = 40
    A = torch.ones(K * 300 + 64, device="cuda")
    G = torch.full((K * 300 + 64,), 3.0, device="cuda")
    C = torch.full((300 * 300,), 7.0, device="cuda")

    def call(M, N, a_off=0, flags=0):
        return lib.gaib_sgemm_split_tn(h, M, N, K, A.data_ptr() + a_off, G.data_ptr(), None, flags, C.data_ptr())

    for M, N in [(6, 16), (16, 47), (260, 16)]:
        assert call(M, N) == -5 and not ctx.sgemm_split_tn_cover(M, N) and ctx.sgemm_split_tn_parts(M, N, K) == 0, (M, N)
    assert b"gaib_sgemm_ex" in lib.gaib_last_error()
    assert ctx.sgemm_split_tn_cover(16, 16) and ctx.sgemm_split_tn_cover(256, 256) and ctx.sgemm_split_tn_cover(4, 100)
    assert call(16, 16, a_off=4) == -5  # A off a 16-byte boundary
    assert call(16, 16, flags=2) == -5 and call(16, 16, flags=3) == -5  # GAIB_RELU
    torch.cuda.synchronize()
    assert bool((C == 7.0).all()) and bool((G == 3.0).all())
    assert call(16, 16) == 0  # and the covered call does run
    torch.cuda.synchronize()
    assert bool((C[: 16 * 16] == 3.0 * K).all()) and bool((C[16 * 16:] == 7.0).all()) and bool((G == 3.0).all())


def test_switch_routes_covered_weight_gradients_only(ctx):
    gen = torch.Generator().manual_seed(4)
    K, M = 300, 128
    A = torch.randn(K, M, generator=gen).cuda()
    for N in (128, 47):  # covered; outside the cover (N % 4 != 0)
        G0 = torch.randn(K, N, generator=gen).cuda()
        mask = torch.sign(torch.randn(K, N, generator=gen)).cuda()

        def call(split, opt, masked, direct=False):
            """(C, G afterwards) of the plain or masked weight gradient under the two options, and whether the new kernel ran"""
            G, C = G0.clone(), torch.full((M, N), float("nan"), device="cuda")
            ctx.set_option("sgemm_split", split)
            ctx.set_option("sgemm_split_tn", opt)
            try:
                assert ctx.get_option("sgemm_split_tn") == opt
                ctx.prof_reset()
                ctx.prof_enable(True)
                if direct:
                    ctx.sgemm_split_tn(A, G, C, mask=mask if masked else None)
                elif masked:
                    ctx.sgemm_drelu(A, G, mask, C)
                else:
                    ctx.sgemm(A, G, C, transA=True)
                torch.cuda.synchronize()
                return bits32(C), bits32(G), f"sgemm_split_tn@{M}x{N}x{K}" in ctx.prof_table()
            finally:
                ctx.prof_enable(False)
                ctx.prof_reset()
                ctx.set_option("sgemm_split", 0)
                ctx.set_option("sgemm_split_tn", 0)

        for masked in (False, True):
            off, other, on = call(0, 0, masked), call(1, 0, masked), call(0, 1, masked)
            assert not off[2] and not other[2] and on[2] == (N == 128), (N, masked)
            same_as = call(0, 1, masked, direct=True) if N == 128 else off  # routed: the direct call's bits; not routed: fp32's
            assert torch.equal(on[0], same_as[0]) and torch.equal(on[1], same_as[1]), (N, masked)


@pytest.fixture
def split_on(lctx):  # noqa: F811
    lctx.set_option("sgemm_split", 1)
    lctx.set_option("sgemm_split_tn", 1)
    lctx.prof_reset()
    lctx.prof_enable(True)
    yield lctx
    lctx.prof_enable(False)
    lctx.prof_reset()
    lctx.set_option("sgemm_split", 0)
    lctx.set_option("sgemm_split_tn", 0)


@pytest.mark.parametrize("din,dout,drop,fuse", [(100, 128, 0.0, 1), (256, 256, LR.RATE, 0)], ids=["100x128", "256x256-drop-unfused"])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_gcn_and_sage_layers_stay_exact(split_on, layer, kind, din, dout, drop, fuse):  # noqa: F811
    """integer operands on the regular graph: a whole layer, its weight gradients included, is exact in fp32, whichever planes
    carry it (the cells of test_gpu_sgemm_split.py)"""
    split_on.set_option("spmm_fuse", fuse)
    try:
        d = layer(kind, din, dout, 1, True, drop)
        out = d.forward()
        ref = d.reference(d.ops.g, d.checked_mask() if drop else None)
        d.check_forward(out, ref, " [sgemm_split_tn]")
        d.check_backward(d.backward(out, d.ops.g), ref, " [sgemm_split_tn]")
    finally:
        split_on.set_option("spmm_fuse", 1)  # (its default; it cannot be read back)
    keys = sorted(split_on.prof_table())
    print(kind, din, dout, keys)
    assert any(k.startswith("sgemm_split_tn@") for k in keys), keys


def test_trainer_with_split_weight_gradients(tmp_path):
    """SAGE, two layers at hidden 256: the loss curve under GAIB_GEMM_DTYPE=split_wgrad against the fp32 products' with the
    tolerance the project gives GAIB_GEMM_DTYPE=split (2 % of the fp32 loss at every epoch)"""
    root = make_dataset(tmp_path)
    cmd = [str(ROOT / "bin" / "gpu_train_sage"), "cora", "20", "2", "softmax", "256", "0", "0", "0.01", "2", "0", "4", "0"]
    runs = {}
    for dt in ("fp32", "split_wgrad"):
        env = dict(os.environ, DATASET_PATH=root, GAIB_GEMM_DTYPE=dt, GAIB_EPOCH_GRAPH="0", GAIB_EPOCH_LOSSES="1")
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("dense products: split bf16 planes, weight gradients included" in r.stdout) == (dt == "split_wgrad"), r.stdout[:2000]
        runs[dt] = [float(v) for v in re.search(r"epoch_losses ([0-9eE.+\- ]+)", r.stdout + r.stderr).group(1).split()]
        assert len(runs[dt]) == 20, runs[dt]
    s, f = runs["split_wgrad"], runs["fp32"]
    print("split_wgrad:", s, "fp32:", f)
    assert s[-1] < s[0] * 0.9, s
    assert all(abs(x - y) <= 0.02 * y for x, y in zip(s, f)), (s, f)
