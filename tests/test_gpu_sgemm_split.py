"""GPU suite, gaib_sgemm_split: the fp32 dense product on the bf16 matrix cores with both operands split exactly into three bf16
planes.  Exact cases (one term per output; integer sums that need the cross planes), the derived bound on random data, the
refusals and the switch sgemm_split of gaib_sgemm_ex, the GCN / SAGE / GAT layers and the trainer under the option."""
import os
import re
import subprocess
from functools import lru_cache
from pathlib import Path

import pytest
import torch

import layer_ref64 as LR
from test_gpu_bf16 import make_dataset
from test_gpu_gat_layers64 import graph, run_cell  # noqa: F401  (the GAT graph's fixture, one cell to that file's rule)
from test_gpu_layers_exact import graphs, layer, lctx  # noqa: F401  (fixtures of the exact layer cells)

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
U32 = 2.0 ** -23
GUARD = 64  # floats of NaN bits in front of and behind A and C
BASIC = [(1, 4, 4), (17, 16, 16), (33, 100, 128), (257, 128, 128), (300, 256, 256)]  # (M, K, N); 100: a half chunk past K
SHAPES = BASIC + ["ring"]
IDS = ["x".join(map(str, s)) if s != "ring" else s for s in SHAPES]


def resolve(ctx, shape):
    """a basic shape as it is; "ring": N = 256 and an M at which some waves run one full round of the ring plus one tile and the others plus two: the steady
    loop and both drain lengths.  The launcher's grid rule (sgemm_split.hip, sgemm_split_grid): 4 slabs of 64 columns, row groups
    nrg = max(8, num_cus / 4 / 8 * 8) of four waves, wave w of W = 4 nrg takes the 16-row tiles w, w + W, ...  With 4 W + W / 2
    tiles the first half of the waves has 5 tiles, the second 4 (ring of 3); the last tile is partial (M = 16 tiles - 5)."""
    if shape != "ring":
        return shape
    nrg = max(8, ctx.get_option("num_cus") // 4 // 8 * 8)
    W = 4 * nrg
    tiles = 4 * W + W // 2
    per_wave = {(tiles - w + W - 1) // W for w in range(W)}
    assert per_wave == {3 + 1, 3 + 2}, per_wave
    return (16 * tiles - 5, 256, 256)


def bits32(t):
    return t.contiguous().view(torch.int32)


def run(ctx, a, b, transB, lda=None, C0=None, relu=False):
    """gaib_sgemm_split on A [M x K] laid out at stride lda and B [K x N] (handed over as [N x K] with transB).  The pad columns
    of A and a guard band round A and C hold NaN bits: a NaN in the result means one of them was consumed."""
    (M, K), N = a.shape, b.shape[1]
    lda = lda or K
    rawA = torch.full((2 * GUARD + M * lda,), float("nan"))
    rawA[GUARD:GUARD + M * lda].view(M, lda)[:, :K] = a
    rawA = rawA.cuda()
    rawC = torch.full((2 * GUARD + M * N,), float("nan"), device="cuda")
    Cm = rawC[GUARD:GUARD + M * N].view(M, N)
    if C0 is not None:
        Cm.copy_(C0)
    Bd = (b.t().contiguous() if transB else b.contiguous()).cuda()
    ctx.sgemm_split(rawA[GUARD:GUARD + M * lda].view(M, lda), Bd, Cm, K=K, transB=transB, accum=C0 is not None, relu=relu)
    torch.cuda.synchronize()
    assert bool(torch.isnan(rawC[:GUARD]).all()) and bool(torch.isnan(rawC[GUARD + M * N:]).all()), "C's guard band was written"
    return Cm.cpu()


# ---- 1: exact, one term per output ------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def one_term(M, K, N):
    """row i has its one non-zero in column k = i % K, at exponent -90, 0 or 126.  Even k: A holds all 24 mantissa bits and row k of
    B is +-2^e; odd k: A is +-2^e and row k of B holds a full mantissa (lowest bit set) times 2^e -- each product has 24 bits"""
    gen = torch.Generator().manual_seed(100 + M)
    i = torch.arange(M)
    k = i % K
    sgn = torch.randint(0, 2, (M,), generator=gen).double() * 2 - 1
    mant = torch.where(k % 2 == 0, torch.tensor(2.0 - 2.0 ** -23, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    a = torch.zeros(M, K)
    a[i, k] = (sgn * mant * torch.exp2(torch.tensor([-90.0, 0.0, 126.0], dtype=torch.float64)[i % 3])).float()
    full = ((torch.randint(0, 1 << 23, (K, N), generator=gen) | 1) + (1 << 23)).double() * 2.0 ** -23  # [1, 2), 24 bits
    scale = torch.exp2(torch.randint(-20, 1, (K, N), generator=gen).double()) * (torch.randint(0, 2, (K, N), generator=gen) * 2 - 1)
    b = (torch.where((torch.arange(K) % 2 == 0)[:, None], torch.ones(K, N, dtype=torch.float64), full) * scale).float()
    want = a.double() @ b.double()
    assert bool(torch.isfinite(want).all()) and torch.equal(want.float().double(), want)  # the fp64 product is an fp32 value
    return a, b, want.float()


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("transB", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_term_per_output_is_exact(ctx, shape, transB, pad):
    M, K, N = resolve(ctx, shape)
    a, b, want = one_term(M, K, N)
    got = run(ctx, a, b, transB, lda=K + pad)
    assert not torch.isnan(got).any(), "a NaN in the output: a pad column (K .. lda - 1) or the guard band was consumed"
    bad = bits32(got) != bits32(want)
    assert not bad.any(), (shape, transB, pad, int(bad.sum()), got[bad][:4], want[bad][:4])


# ---- 2: exact, integer sums that need the cross planes ----------------------------------------------------------------------
@lru_cache(maxsize=None)
def int_case(kind, M, K, N):
    """a: three 21-bit odd entries per row of A against B = +-1 (A's third plane); b: the mirror image; c: three 11-bit odd
    entries per row against a dense odd 11-bit B (plane 1 x plane 1)"""
    gen = torch.Generator().manual_seed(7 * M + K + N)
    bits_a, bits_b = {"a": (21, 1), "b": (1, 21), "c": (11, 11)}[kind]

    def odd(shape, bits):
        mag = torch.randint(1 << (bits - 2), 1 << (bits - 1), shape, generator=gen) * 2 + 1 if bits > 1 else torch.ones(shape, dtype=torch.int64)
        return (mag * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()

    a = torch.zeros(M, K)
    i = torch.arange(M)
    for col in (i, 7 * i + 3, 13 * i + 5):
        a[i, col % K] = odd((M,), bits_a)
    b = odd((K, N), bits_b)
    c0 = torch.randint(-(1 << 20) + 1, 1 << 20, (M, N), generator=gen).float()
    assert float((a.double().abs() @ b.double().abs() + c0.double().abs()).max()) < 2 ** 24  # every partial sum is exact
    return a, b, c0, a.double() @ b.double()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("accum", [False, True])
def test_integer_sums_are_exact(ctx, accum, relu):
    for kind in "abc":
        for n, shape in enumerate(SHAPES):
            M, K, N = resolve(ctx, shape)
            a, b, c0, prod = int_case(kind, M, K, N)
            want = prod + (c0.double() if accum else 0)
            want = want.clamp(min=0) if relu else want
            got = run(ctx, a, b, bool(n % 2), C0=c0 if accum else None, relu=relu)
            bad = got.double() != want
            assert not bad.any(), (kind, shape, accum, relu, int(bad.sum()), got[bad][:4], want[bad][:4])


# ---- 3: random data, derived bound ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("transB", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_data_within_the_bound(ctx, shape, transB, accum):
    """test_gpu_gemm_bf16's bound with 9 K exact terms in place of 3 K: 9 K + 1 terms, one ulp per addition,
    sum_t |w_t| <= 1.004 |B| (the truncated planes of A sum to |A|): |C - C64| <= (9 K + 4) 2^-23 (|A| |B| + |C0|)"""
    M, K, N = resolve(ctx, shape)
    gen = torch.Generator().manual_seed(M + K)
    a = torch.randn(M, K, generator=gen)
    b = (torch.rand(K, N, generator=gen) * 2 - 1) * (6.0 / (K + N)) ** 0.5  # Glorot range
    c0 = torch.randn(M, N, generator=gen) if accum else None
    got = run(ctx, a, b, transB, C0=c0)
    c64 = a.double() @ b.double() + (c0.double() if accum else 0)
    bound = (9 * K + 4) * U32 * (a.double().abs() @ b.double().abs() + (c0.double().abs() if accum else 0))
    err = (got.double() - c64).abs()
    print(f"{shape} transB={transB} accum={accum}: worst err / bound = {float((err / bound.clamp(min=1e-300)).max()):.4f}")
    assert bool((err <= bound).all()), (shape, accum, float((err - bound).max()))
    assert torch.equal(bits32(run(ctx, a, b, transB, C0=c0)), bits32(got))  # the same call twice: the same bits


# ---- 4: refusals leave C untouched; the switch of gaib_sgemm_ex -------------------------------------------------------------
def test_refusals_leave_c_untouched(ctx):
    lib, h = ctx.lib, ctx.h
    M = 40
    raw = torch.ones(M * 300 + 64, device="cuda")
    B = torch.ones(300 * 300, device="cuda")
    Craw = torch.full((M * 300 + 64,), 7.0, device="cuda")

    def call(N, K, lda, a_off=0, transB=0):
        return lib.gaib_sgemm_split(h, transB, M, N, K, lda, raw.data_ptr() + a_off, B.data_ptr(), 0, Craw.data_ptr())

    for N, K, lda in [(16, 6, 8), (47, 16, 16), (16, 260, 260)]:
        for tb in (0, 1):
            assert call(N, K, lda, transB=tb) == -5 and not ctx.sgemm_split_cover(N, K, lda, bool(tb)), (N, K, lda)
    assert b"gaib_sgemm_ex" in lib.gaib_last_error()
    assert ctx.sgemm_split_cover(16, 16, 16) and ctx.sgemm_split_cover(256, 256, 260, True) and ctx.sgemm_split_cover(4, 4, 4)
    assert call(16, 16, 16, a_off=4) == -5  # A off a 16-byte boundary
    ctx.set_option("sgemm_split_kernel", 0)
    try:
        assert call(16, 16, 16) == -5 and not ctx.sgemm_split_cover(16, 16, 16)
    finally:
        ctx.set_option("sgemm_split_kernel", 1)
    torch.cuda.synchronize()
    assert bool((Craw == 7.0).all())
    assert call(16, 16, 16) == 0  # and the covered call does run
    torch.cuda.synchronize()
    assert bool((Craw[: M * 16] == 16.0).all()) and bool((Craw[M * 16:] == 7.0).all())


def test_switch_routes_covered_products_only(ctx):
    gen = torch.Generator().manual_seed(4)
    A = torch.randn(300, 128, generator=gen).cuda()
    out = {}
    for N in (128, 47):  # covered; outside the cover (N % 4 != 0)
        B = torch.randn(128, N, generator=gen).cuda()
        for opt in (0, 1):
            ctx.set_option("sgemm_split", opt)
            try:
                assert ctx.get_option("sgemm_split") == opt
                ctx.prof_reset()
                ctx.prof_enable(True)
                out[N, opt] = ctx.sgemm(A, B, torch.full((300, N), float("nan"), device="cuda"), relu=True)
                torch.cuda.synchronize()
                keys = sorted(ctx.prof_table())
                assert (f"sgemm_split@300x{N}x128" in keys) == (opt == 1 and N == 128), keys
            finally:
                ctx.prof_enable(False)
                ctx.prof_reset()
                ctx.set_option("sgemm_split", 0)
        if N == 128:
            direct = ctx.sgemm_split(A, B, torch.full((300, N), float("nan"), device="cuda"), relu=True)
            assert torch.equal(bits32(out[N, 1]), bits32(direct))
        else:
            assert torch.equal(bits32(out[N, 1]), bits32(out[N, 0]))


# ---- 5: the layers and the trainer under the option -------------------------------------------------------------------------
@pytest.fixture
def split_on(lctx):  # noqa: F811
    lctx.set_option("sgemm_split", 1)
    lctx.prof_reset()
    lctx.prof_enable(True)
    yield lctx
    lctx.prof_enable(False)
    lctx.prof_reset()
    lctx.set_option("sgemm_split", 0)


@pytest.mark.parametrize("din,dout,drop,fuse", [(100, 128, 0.0, 1), (256, 256, LR.RATE, 0)], ids=["100x128", "256x256-drop-unfused"])
@pytest.mark.parametrize("kind", LR.KINDS)
def test_gcn_and_sage_layers_stay_exact(split_on, layer, kind, din, dout, drop, fuse):  # noqa: F811
    """integer operands on the regular graph: a whole layer is exact in fp32, whichever planes carry it.  (256 -> 256 on this
    small graph is fused into the aggregation in both directions: spmm_fuse = 0 sends its products through gaib_sgemm_ex)"""
    split_on.set_option("spmm_fuse", fuse)
    try:
        d = layer(kind, din, dout, 1, True, drop)
        out = d.forward()
        ref = d.reference(d.ops.g, d.checked_mask() if drop else None)
        d.check_forward(out, ref, " [sgemm_split]")
        d.check_backward(d.backward(out, d.ops.g), ref, " [sgemm_split]")
    finally:
        split_on.set_option("spmm_fuse", 1)  # (its default; it cannot be read back)
    keys = sorted(split_on.prof_table())
    print(kind, din, dout, keys)
    assert any(k.startswith("sgemm_split@") for k in keys), keys


def test_gat_layer_against_fp64(split_on, graph):  # noqa: F811
    run_cell(split_on, graph, "rule", 100, 64, 8, True, 1, 0.0)
    assert any(k.startswith("sgemm_split@") for k in split_on.prof_table()), sorted(split_on.prof_table())


def test_trainer_with_split_products(tmp_path):
    """SAGE, two layers at hidden 256 on fp32 tables: 96 -> 256 is covered; the loss curve against the fp32 products' with the
    tolerance test_gpu_gemm_bf16's trainer test gives GAIB_GEMM_DTYPE=bf16 (2 % of the fp32 loss), here at every epoch"""
    root = make_dataset(tmp_path)
    cmd = [str(ROOT / "bin" / "gpu_train_sage"), "cora", "20", "2", "softmax", "256", "0", "0", "0.01", "2", "0", "4", "0"]
    runs = {}
    for dt in ("fp32", "split"):
        env = dict(os.environ, DATASET_PATH=root, GAIB_GEMM_DTYPE=dt, GAIB_EPOCH_GRAPH="0", GAIB_EPOCH_LOSSES="1")
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("dense products: split bf16 planes" in r.stdout) == (dt == "split"), r.stdout[:2000]
        runs[dt] = [float(v) for v in re.search(r"epoch_losses ([0-9eE.+\- ]+)", r.stdout + r.stderr).group(1).split()]
        assert len(runs[dt]) == 20, runs[dt]
    s, f = runs["split"], runs["fp32"]
    print("split:", s, "fp32:", f)
    assert s[-1] < s[0] * 0.9, s
    assert all(abs(x - y) <= 0.02 * y for x, y in zip(s, f)), (s, f)
