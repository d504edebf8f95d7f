"""GPU suite: the fp32 dense products (csrc/sgemm.hip, csrc/sgemm_skinny.hip) held to EXACT sums at every alignment.

tests/exact.py has the method and the table: operands are small integers, every partial sum in any order is an integer below
2^24 (asserted from the data), so every correct fp32 kernel returns the bits of the fp64 reference and the comparison is
torch.equal -- no tolerance.  E.DENSE_CASES has one row per dispatch branch and shape, with the rule that sends it there; a row
runs under each sgemm_variant it lists, with (accum, relu) in {(0, 0), (1, 1)} (the masked form: accum 0 and 1), and with
A, B, C (and the mask) placed 0, 1 or 2 floats past a 16-byte boundary inside guarded buffers that end where the operand ends.

Every run asserts: the call returns OK (a misaligned operand falls to another kernel, never to an error); C equals the
reference by value (so -0 equals +0: the sign of a zero is not part of the contract); C's guards keep their bits; A and B keep
theirs -- in the masked form G comes back as G0 * (mask > 0) bit for bit and the mask is unchanged.  Once per row and variant
the shape also runs twice on N(0, 1) operands: the same bits both times, within rel_err 2e-5 of fp64 (test_gpu_ops.py's bound)."""
import numpy as np
import pytest
import torch

import exact as E
from graphaibench_amd import capi

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


def run_plain(ctx, ops, dev, accum, relu, offs, what):
    oa, ob, oc = offs
    tA, tB = E.FORMS[ops.form]
    a, b = E.placed(dev["A"], oa), E.placed(dev["B"], ob)
    c = E.placed(dev["C0"] if accum else dev["nan"], oc, fill=E.OUT_BITS)
    ctx.sgemm(a, b, c, transA=tA, transB=tB, accum=accum, relu=relu)   # raises unless GAIB_OK
    ctx.sync()
    assert E.guards_intact(c, oc, fill=E.OUT_BITS), f"{what}: C's guards were written"
    assert torch.equal(bits(a), bits(dev["A"])) and E.guards_intact(a, oa), f"{what}: A changed"
    assert torch.equal(bits(b), bits(dev["B"])) and E.guards_intact(b, ob), f"{what}: B changed"
    return c


def run_masked(ctx, ops, dev, accum, offs, what):
    oa, ob, oc, om = offs
    a, g, m = E.placed(dev["A"], oa), E.placed(dev["B"], ob), E.placed(dev["mask"], om)
    c = E.placed(dev["C0"] if accum else dev["nan"], oc, fill=E.OUT_BITS)
    ctx.sgemm_drelu(a, g, m, c, accum=accum)
    ctx.sync()
    assert E.guards_intact(c, oc, fill=E.OUT_BITS), f"{what}: C's guards were written"
    assert torch.equal(bits(a), bits(dev["A"])) and E.guards_intact(a, oa), f"{what}: A changed"
    assert torch.equal(bits(m), bits(dev["mask"])) and E.guards_intact(m, om), f"{what}: the mask changed"
    assert E.guards_intact(g, ob), f"{what}: G's guards were written"
    assert torch.equal(bits(g), bits(dev["Gm"])), f"{what}: G is not G0 * (mask > 0) bit for bit"
    return c


def mismatch(c, ref, what):
    bad = (c != ref).nonzero()
    i = tuple(int(v) for v in bad[0])
    return f"{what}: {bad.shape[0]} of {c.numel()} entries differ from the exact sum, first at {i}: {c[i].item()!r} for {ref[i].item()!r}"


def normal_twice(ctx, form, M, N, K, what):
    """N(0, 1) operands, aligned: the same bits twice, and rel_err < 2e-5 against fp64"""
    gen = torch.Generator(device="cuda").manual_seed(M + 3 * N + 7 * K)
    sa, sb = E.dense_shapes(form, M, N, K)
    tA, tB = E.FORMS[form]
    A, B = (torch.randn(s, device="cuda", generator=gen) for s in (sa, sb))
    mask = torch.randn(sb, device="cuda", generator=gen) if form == "mask" else None
    Bm = B if mask is None else torch.where(mask > 0, B, torch.zeros_like(B))
    ref = (A.double().t() if tA else A.double()) @ (Bm.double().t() if tB else Bm.double())
    got = []
    for _ in range(2):
        c = torch.full((M, N), float("nan"), device="cuda")
        if mask is None:
            ctx.sgemm(A, B, c, transA=tA, transB=tB)
        else:
            ctx.sgemm_drelu(A, B.clone(), mask, c)
        got.append(c)
    assert torch.equal(bits(got[0]), bits(got[1])), f"{what}: two runs of the same product differ in their bits"
    err = ((got[0].double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
    print(f"{what}: N(0,1) rel_err {err:.3e}")
    assert err < 2e-5, f"{what}: N(0,1) rel_err {err:.3e}"


@pytest.mark.parametrize("case", E.DENSE_CASES, ids=[E.dense_id(c) for c in E.DENSE_CASES])
def test_dense_exact(ctx, case):
    branch, form, M, N, K, variants = case
    ops = E.dense_operands(form, M, N, K, seed=1)
    dev = {k: torch.from_numpy(getattr(ops, k)).cuda() for k in ("A", "B", "C0")}
    dev["nan"] = torch.full((M, N), float("nan"), device="cuda")   # without accum nothing of C's pre-fill may survive
    masked = form == "mask"
    if masked:
        dev["mask"] = torch.from_numpy(ops.mask).cuda()
        dev["Gm"] = torch.from_numpy(E.effective_b(ops)).cuda()
    modes = ((False, False), (True, False)) if masked else ((False, False), (True, True))
    refs = {}
    for accum, relu in modes:
        r64 = E.dense_ref(ops, accum, relu, device="cuda")
        refs[accum, relu] = r64.float()
        assert torch.equal(refs[accum, relu].double(), r64)   # the cast is exact
    try:
        for sv in variants:
            ctx.set_option("sgemm_variant", sv)
            for accum, relu in modes:
                for offs in (E.OFFSETS_MASK if masked else E.OFFSETS):
                    what = f"{branch}: {form} {M} x {N} x {K} variant {sv} accum {accum} relu {relu} offsets {offs}"
                    c = run_masked(ctx, ops, dev, accum, offs, what) if masked else run_plain(ctx, ops, dev, accum, relu, offs, what)
                    ref = refs[accum, relu]
                    assert torch.equal(c, ref), mismatch(c, ref, what)
            normal_twice(ctx, form, M, N, K, f"{branch}: {form} {M} x {N} x {K} variant {sv}")
    finally:
        ctx.set_option("sgemm_variant", 0)


def test_tt_stays_refused(ctx):
    """the one form that is an error: transA && transB (not on the GNN path)"""
    A, B, C = (torch.ones(8, 8, device="cuda") for _ in range(3))
    with pytest.raises(capi.GaibError):
        ctx.sgemm(A, B, C, transA=True, transB=True)
