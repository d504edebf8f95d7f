"""GPU suite, gaib_gemm_bf16: the dense product of a bf16 table with fp32 weights that are split exactly into three bf16
planes on the device.  Exact cases (one term per output; integer sums that need the third plane), the derived bound on random
data, the refusals, determinism, a recorded call, the SAGE layers under the option gemm_bf16, and the trainer with
GAIB_GEMM_DTYPE."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from graphaibench_amd import capi, layers as L
from test_gpu_bf16 import lctx, make_dataset  # noqa: F401  (fixture, dataset builder of the bf16 trainer tests)
from util import random_graph

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
U32 = 2.0 ** -23
NAN_BITS = 0x7FC0
SHAPES = [(1, 8, 4), (17, 16, 16), (257, 128, 128), (300, 256, 256), (4099, 64, 100)]  # (M, K, N)


def bits32(t):
    return t.contiguous().view(torch.int32)


def table(a32, lda):
    """fp32 [M x K] of bf16-representable values -> the bf16 table [M x lda] on the device, pad columns filled with NaN bits"""
    M, K = a32.shape
    t = torch.full((M, lda), NAN_BITS, dtype=torch.int16).view(torch.bfloat16)
    t[:, :K] = a32.to(torch.bfloat16)
    assert torch.equal(t[:, :K].to(torch.float32), a32)
    return t.cuda()


def run(ctx, A, B, K, transB, C0=None, relu=False):
    """gaib_gemm_bf16 on table A [M x lda] and B [K x N] (handed over as [N x K] with transB); C0: accumulate onto it"""
    M, N = A.shape[0], B.shape[1]
    Bd = (B.t().contiguous() if transB else B.contiguous()).cuda()
    Cm = C0.clone().cuda() if C0 is not None else torch.full((M, N), float("nan"), device="cuda")
    ctx.gemm_bf16(A, Bd, Cm, K=K, transB=transB, accum=C0 is not None, relu=relu)
    torch.cuda.synchronize()
    return Cm.cpu()


# ---- 1: exact, one term per output ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_term():
    out = {}
    for M, K, N in SHAPES:
        gen = torch.Generator().manual_seed(100 + M)
        a = torch.zeros(M, K)
        e = torch.randint(-6, 7, (M,), generator=gen).to(torch.float32)
        sgn = torch.randint(0, 2, (M,), generator=gen).to(torch.float32) * 2 - 1
        i = torch.arange(M)
        a[i, i % K] = sgn * torch.exp2(e)
        b = (torch.randn(K, N, generator=gen).view(torch.int32) & ~3).view(torch.float32)  # two lowest mantissa bits cleared
        want = (a.double() @ b.double()).to(torch.float32)
        assert torch.equal(want.double(), a.double() @ b.double())  # (one term per output: the fp64 product is an fp32 value)
        out[(M, K, N)] = (a, b, want)
    return out


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("transB", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_term_per_output_is_exact(ctx, one_term, shape, transB, pad):
    M, K, N = shape
    a, b, want = one_term[shape]
    got = run(ctx, table(a, K + pad), b, K, transB)
    assert not torch.isnan(got).any(), "a NaN in the output: a pad column (K .. lda - 1) was read"
    bad = bits32(got) != bits32(want)
    assert not bad.any(), (shape, transB, pad, int(bad.sum()), got[bad][:4], want[bad][:4])


# ---- 2: exact, integer sums that need the third plane -----------------------------------------------------------------------
def int_case(M, K, N):
    gen = torch.Generator().manual_seed(7 * M + K + N)
    a = torch.zeros(M, K)
    i = torch.arange(M)
    for col in (i, 7 * i + 3, 13 * i + 5):
        a[i, col % K] = torch.randint(0, 2, (M,), generator=gen).to(torch.float32) * 2 - 1
    mag = torch.randint(1 << 19, 1 << 20, (K, N), generator=gen) * 2 + 1  # odd, 21 bits
    b = (mag * (torch.randint(0, 2, (K, N), generator=gen) * 2 - 1)).to(torch.float32)
    c0 = torch.randint(-(1 << 20) + 1, 1 << 20, (M, N), generator=gen).to(torch.float32)
    prod = a.double() @ b.double()  # integers below 2^24: exact
    return a, b, c0, prod


@pytest.mark.parametrize("M", [512, 4099])
@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("K", [64, 256])
def test_integer_sums_are_exact(ctx, M, K, N):
    a, b, c0, prod = int_case(M, K, N)
    A = table(a, K)
    for accum in (False, True):
        for relu in (False, True):
            want = prod + (c0.double() if accum else 0)
            if relu:
                want = want.clamp(min=0)
            got = run(ctx, A, b, K, bool((M + K + N) // 64 % 2), c0 if accum else None, relu)
            bad = got.double() != want
            assert not bad.any(), (M, K, N, accum, relu, int(bad.sum()), got[bad][:4], want[bad][:4])


# ---- 3: random data, derived bound ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("transB", [False, True])
@pytest.mark.parametrize("shape", SHAPES + [(1000, 136, 48)], ids=lambda s: "x".join(map(str, s)))
def test_random_data_within_the_bound(ctx, shape, transB, accum):
    """3 K + 1 exact terms, one ulp per addition (covers a truncating accumulator), sum_t |w_t| <= 1.004 |B|:
    |C - C64| <= (3 K + 4) 2^-23 (|A| |B| + |C0|) element by element"""
    M, K, N = shape
    gen = torch.Generator().manual_seed(M + K)
    a = torch.randn(M, K, generator=gen).to(torch.bfloat16).to(torch.float32)
    r = (6.0 / (K + N)) ** 0.5
    b = (torch.rand(K, N, generator=gen) * 2 - 1) * r  # Glorot range
    c0 = torch.randn(M, N, generator=gen) if accum else None
    got = run(ctx, table(a, K), b, K, transB, c0)
    c64 = a.double() @ b.double() + (c0.double() if accum else 0)
    bound = (3 * K + 4) * U32 * (a.double().abs() @ b.double().abs() + (c0.double().abs() if accum else 0))
    err = (got.double() - c64).abs()
    print(f"{shape} transB={transB} accum={accum}: worst err / bound = {float((err / bound.clamp(min=1e-300)).max()):.4f}")
    assert bool((err <= bound).all()), (shape, accum, float((err - bound).max()))


# ---- 4: refusals leave C untouched ------------------------------------------------------------------------------------------
def test_refusals_leave_c_untouched(ctx):
    lib, h = ctx.lib, ctx.h
    M = 40
    raw = torch.zeros(M * 300 + 64, dtype=torch.bfloat16, device="cuda")
    B = torch.ones(300 * 300, device="cuda")
    Craw = torch.full((M * 300 + 64,), 7.0, device="cuda")

    def call(N, K, lda, a_off=0, c_off=0, transB=0):
        return lib.gaib_gemm_bf16(h, transB, M, N, K, lda, raw.data_ptr() + a_off, B.data_ptr(), 0, Craw.data_ptr() + c_off)

    shape_cases = [(16, 12, 16), (6, 16, 16), (260, 16, 16), (16, 264, 264), (16, 16, 8), (16, 16, 20)]  # (N, K, lda)
    for N, K, lda in shape_cases:
        for tb in (0, 1):
            assert call(N, K, lda, transB=tb) == -5, (N, K, lda)
            assert not ctx.gemm_bf16_cover(N, K, lda, bool(tb)), (N, K, lda)
    assert b"gaib_sgemm_ex" in lib.gaib_last_error()
    assert ctx.gemm_bf16_cover(16, 16, 16) and ctx.gemm_bf16_cover(256, 256, 264, True) and ctx.gemm_bf16_cover(4, 8, 8)
    assert call(16, 16, 16, a_off=4) == -5 and call(16, 16, 16, c_off=4) == -5  # misaligned by 4 bytes
    ctx.set_option("gemm_bf16_kernel", 0)
    try:
        assert call(16, 16, 16) == -5 and not ctx.gemm_bf16_cover(16, 16, 16)
    finally:
        ctx.set_option("gemm_bf16_kernel", 1)
    assert lib.gaib_gemm_bf16(h, 0, 0, 16, 16, 16, raw.data_ptr(), B.data_ptr(), 0, Craw.data_ptr()) == 0  # M == 0
    torch.cuda.synchronize()
    assert bool((Craw == 7.0).all())
    assert call(16, 16, 16) == 0  # and the covered call does run
    torch.cuda.synchronize()
    assert bool((Craw[: M * 16] == 0.0).all()) and bool((Craw[M * 16:] == 7.0).all())


# ---- 5: determinism, and a recorded call ------------------------------------------------------------------------------------
def test_same_bits_twice_and_when_recorded(ctx):
    M, K, N = 4099, 256, 256
    gen = torch.Generator().manual_seed(5)
    A = torch.randn(M, K, generator=gen).to(torch.bfloat16).cuda()
    B = (torch.randn(N, K, generator=gen) * 0.1).cuda()
    C0 = torch.randn(M, N, generator=gen).cuda()
    outs = []
    for _ in range(2):
        Cm = C0.clone()
        ctx.gemm_bf16(A, B, Cm, transB=True, accum=True, relu=True)
        torch.cuda.synchronize()
        outs.append(Cm)
    assert torch.equal(bits32(outs[0]), bits32(outs[1]))
    s = capi.Context(0)  # a context on a stream of its own (the null stream cannot be recorded)
    s.own_stream()
    try:
        Cm = C0.clone()
        torch.cuda.synchronize()
        s.capture_begin()
        s.gemm_bf16(A, B, Cm, transB=True, accum=True, relu=True)
        ex = s.capture_end()
        assert ex.nodes >= 1
        ex.launch()
        s.sync()
        assert torch.equal(bits32(Cm), bits32(outs[0]))
        ex.close()
    finally:
        s.close()


# ---- 5b: subnormal operands (the finding DESIGN.md 8.2 and include/gaib.h record) ----------------------------------------------
SUBNORMAL = [  # (table bits, weight, C0 or None, the exact result)
    (0x0001, 2.0 ** 100, None, 2.0 ** -33),    # a subnormal table entry 2^-133
    (0x0040, 2.0 ** 100, None, 2.0 ** -27),    # 2^-127
    (0x8040, 2.0 ** 100, None, -(2.0 ** -27)),
    (0x7180, 2.0 ** -130, None, 2.0 ** -30),   # 2^100 times a weight whose plane w0 is a subnormal bf16
    (0x1C80, 2.0 ** -70, None, 2.0 ** -140),   # a subnormal fp32 result
    (0x0000, 1.0, 2.0 ** -140, 2.0 ** -140),   # a subnormal fp32 C input
    (0x5D80, 2.0 ** -120 * (1 + 2.0 ** -9), None, 2.0 ** -60 * (1 + 2.0 ** -9)),  # 2^60: the plane w1 = 2^-129 is subnormal
]


@pytest.mark.parametrize("case", SUBNORMAL, ids=[f"{c[0]:04x}" for c in SUBNORMAL])
def test_subnormal_operands_are_kept(ctx, case):
    """one term per output: the bf16 MFMA flushes neither subnormal bf16 inputs (table entries, planes) nor subnormal fp32
    results or C inputs -- each product comes out exactly"""
    abits, w, c0, want = case
    M, K, N = 32, 32, 16
    A = torch.zeros(M, K, dtype=torch.int16)
    A[:, 0] = abits - 0x10000 if abits >= 0x8000 else abits
    B = torch.zeros(K, N)
    B[0, :] = w
    assert float(B[0, 0]) == w  # (representable in fp32)
    C0 = torch.full((M, N), c0) if c0 is not None else None
    got = run(ctx, A.view(torch.bfloat16).cuda(), B, K, False, C0)
    assert bool((got.double() == want).all()), (case, float(got[0, 0]))


# ---- 6: the layers under the option gemm_bf16 -------------------------------------------------------------------------------
NV = 300


def rounded(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(torch.float32)


def layer_step(lctx, kind, din, dout, act, gemm16, fixed_out=None):
    """one level-1 layer on a random whole graph, agg_bf16 = 1: forward, backward (its d_relu mask taken from `fixed_out`, so
    that both settings mask alike), the profile table of the step"""
    rp, ci = random_graph(NV, 8, seed=3)
    x, gin = rounded((NV, din), 1), rounded((NV, dout), 2)
    wn, ws = rounded((din, dout), 3, 0.08) + 2.0 ** -12, rounded((din, dout), 4, 0.08) + 2.0 ** -13  # (not bf16-representable)
    lctx.set_option("agg_bf16", 1)
    lctx.set_option("gemm_bf16", gemm16)
    try:
        g_d = L.LGraph.from_host(rp, ci, add_selfloop=(kind == L.GCN))
        ld = L.Layer(kind, 1, NV, din, dout, g_d, act)
        ld.write(L.W_NEIGH, wn.cuda())
        if kind == L.SAGE:
            ld.write(L.W_SELF, ws.cuda())
        ld.write(L.FEAT_IN, x.cuda())
        out = torch.empty(NV, dout, device="cuda")
        grad_out = torch.zeros(NV, din, device="cuda")
        L.sync()
        lctx.prof_reset()
        lctx.prof_enable(True)
        ld.forward(out)
        L.sync()
        fo = out.clone() if fixed_out is None else fixed_out.cuda()
        ld.write(L.GRAD_IN, gin.cuda())
        ld.backward(fo, grad_out)
        L.sync()
        lctx.prof_enable(False)
        prof = lctx.prof_table()
        lctx.prof_reset()
        res = dict(out=out.cpu(), go=grad_out.cpu(), Wg=ld.tensor(L.W_NEIGH_GRAD, (din, dout)).cpu(), prof=prof,
                   x=x, gin=gin, wn=wn, ws=ws, rp=rp, ci=ci)
        if kind == L.SAGE:
            res["Wsg"] = ld.tensor(L.W_SELF_GRAD, (din, dout)).cpu()
        ld.close()
        g_d.close()
        return res
    finally:
        lctx.prof_enable(False)
        lctx.set_option("gemm_bf16", 0)
        lctx.set_option("agg_bf16", 0)


def n_accumulating(prof, M, N, K):
    """accumulating launches among the sgemm rows of this shape (a row's bytes: 4 (M K + K N + M N (1 + accum)) per launch)"""
    row = prof.get(f"sgemm@{M}x{N}x{K}")
    if row is None:
        return 0
    plain = 4.0 * (M * K + K * N + M * N)
    return round((row["bytes"] - row["count"] * plain) / (4.0 * M * N))


@pytest.mark.parametrize("din,dout", [(256, 256), (128, 256)])
def test_sage_layer_self_products_on_the_bf16_table(lctx, din, dout):
    off = layer_step(lctx, L.SAGE, din, dout, True, 0)
    on = layer_step(lctx, L.SAGE, din, dout, True, 1, fixed_out=off["out"])
    # the weight gradients do not go through the new call
    for k in ("Wg", "Wsg"):
        assert torch.equal(bits32(on[k]), bits32(off[k])), k
    # the profile: gemm_bf16 rows instead of the accumulating fp32 products
    tag = f"gemm_bf16@{NV}x{dout}x{din}"
    assert tag in on["prof"] and on["prof"][tag]["count"] >= 1, sorted(on["prof"])
    assert n_accumulating(on["prof"], NV, dout, din) == 0, on["prof"]
    assert not [k for k in off["prof"] if k.startswith("gemm_bf16")], sorted(off["prof"])
    assert n_accumulating(off["prof"], NV, dout, din) >= 1, off["prof"]
    if din == dout:  # backward's g . W_self^T rides the same route
        assert on["prof"][tag]["count"] == 2, on["prof"][tag]
    # out / grad_out: the bound of test 3 on the self term, C0 = the neighbour term
    x, gin, wn, ws = (off[k].double() for k in ("x", "gin", "wn", "ws"))
    rp, ci = off["rp"], off["ci"]
    deg = np.diff(rp).astype(np.float64)
    A = np.zeros((NV, NV))
    np.add.at(A, (np.repeat(np.arange(NV), np.diff(rp)), ci.astype(np.int64)), 1.0)
    Am = torch.from_numpy(A / np.maximum(deg, 1.0)[:, None])   # forward: the row mean
    Amt = torch.from_numpy((A / np.maximum(deg, 1.0)[:, None]).T.copy())  # backward: its transpose
    bound = (3 * din + 4) * U32 * (x.abs() @ ws.abs() + ((Am @ x) @ wn).abs())
    d = (on["out"].double() - off["out"].double()).abs()
    print(f"{din}->{dout} forward: worst difference / bound = {float((d / bound.clamp(min=1e-300)).max()):.4f}")
    assert bool((d <= bound).all()), float((d - bound).max())
    assert not torch.equal(bits32(on["out"]), bits32(off["out"]))  # (another summation order: not the fp32 call's bits)
    g = gin * (off["out"].double() > 0)  # the d_relu mask both backward passes applied
    bound_g = (3 * dout + 4) * U32 * (g.abs() @ ws.abs().t() + ((Amt @ g) @ wn.t()).abs())
    dg = (on["go"].double() - off["go"].double()).abs()
    assert bool((dg <= bound_g).all()), float((dg - bound_g).max())
    if din != dout:  # backward's products are separate fp32 calls there: untouched
        assert torch.equal(bits32(on["go"]), bits32(off["go"]))


@pytest.mark.parametrize("kind,din,dout", [(L.SAGE, 128, 128), (L.GCN, 256, 256)], ids=["sage128_dual_fused", "gcn256"])
def test_other_layers_do_not_change(lctx, kind, din, dout):
    off = layer_step(lctx, kind, din, dout, True, 0)
    on = layer_step(lctx, kind, din, dout, True, 1, fixed_out=off["out"])
    for k in ("out", "go", "Wg") + (("Wsg",) if kind == L.SAGE else ()):
        assert torch.equal(bits32(on[k]), bits32(off[k])), k
    assert {k: v["count"] for k, v in on["prof"].items()} == {k: v["count"] for k, v in off["prof"].items()}
    assert not [k for k in on["prof"] if k.startswith("gemm_bf16")]


# ---- 7: the trainer ---------------------------------------------------------------------------------------------------------
def train(root, layers, epochs, gemm_dtype):
    exe = ROOT / "bin" / "gpu_train_sage"
    assert exe.exists(), "run graphaibench_amd.build"
    cmd = [str(exe), "cora", str(epochs), "2", "softmax", "256", "0", "0", "0.01", str(layers), "0", "4", "0"]
    env = dict(os.environ, DATASET_PATH=root, GAIB_AGG_DTYPE="bf16", GAIB_GEMM_DTYPE=gemm_dtype, GAIB_EPOCH_GRAPH="0", GAIB_EPOCH_LOSSES="1")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    if r.returncode != 0:
        return r, None
    m = re.search(r"epoch_losses ([0-9eE.+\- ]+)", r.stdout + r.stderr)
    losses = [float(v) for v in m.group(1).split()] if m else [float(a) for a in re.findall(r"train_loss ([0-9.]+)", r.stdout)]
    assert len(losses) == epochs, losses
    return r, losses


def test_trainer_with_gemm_dtype(tmp_path):
    """the configuration of test_trainer_with_bf16_tables at hidden 256: two layers, so the new call runs in the first layer's
    forward only (96 -> 256); the output layer (256 -> 7) is outside the cover in both directions and a level-0 layer has no
    grad_out.  The 256 -> 256 products, forward and backward, are covered at the layer level (test 6), not end to end: a
    three-layer run fits its training set within 20 epochs (final losses of 6.4e-5 against 5.7e-5, LEDGER 12.2), where a relative
    bar on the loss measures summation order."""
    root = make_dataset(tmp_path)
    runs = {}
    for dt in ("fp32", "bf16"):
        r, losses = train(root, 2, 20, dt)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "aggregation tables: bf16" in r.stdout
        assert ("dense self products: bf16 tables" in r.stdout) == (dt == "bf16"), r.stdout[:2000]
        runs[dt] = losses
    b, f = runs["bf16"], runs["fp32"]
    print("two layers:", b, f)
    assert b[-1] < b[0] * 0.9, b
    assert abs(b[-1] - f[-1]) <= 0.02 * f[-1], (b[-1], f[-1])
    r, _ = train(root, 2, 20, "fp16")
    assert r.returncode != 0 and "GAIB_GEMM_DTYPE=fp16" in r.stderr, r.stderr[-1000:]
