"""gaib_gemm_bf16 (bf16 table, fp32 weights split exactly into three bf16 planes) against gaib_sgemm_ex on the fp32 table, and
the SAGE 256 -> 256 layer step under agg_bf16 = 1 with the option gemm_bf16 off and on.  One process; the legs of a comparison
alternate call by call (fp32, bf16, fp32, bf16 ...): 3 warm-up and 20 timed iterations per leg, device events around each
call; median (min - max) per leg and the in-run stream-copy rate beside them.  A leg is called faster only if its median beats
the other's by more than the two min - max spreads together.  Fails without a GPU.

    python scripts/gemm_bf16.py OUT.json [ROWS]
"""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from graphaibench_amd import capi, layers as L, synth  # noqa: E402

ROWS = int(sys.argv[2]) if len(sys.argv) > 2 else 2_449_029
ITERS, WARM = 20, 3


def alternate(legs):
    """legs: {name: callable}; -> {name: dict(median_ms, min_ms, max_ms, n)}, the legs taking turns"""
    for _ in range(WARM):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    evs = {k: [] for k in legs}
    for _ in range(ITERS):
        for k, f in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, v in evs.items():
        ts = sorted(a.elapsed_time(b) for a, b in v)
        out[k] = dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1], n=len(ts))
    return out


def verdict(new, old):
    spread = (new["max_ms"] - new["min_ms"]) + (old["max_ms"] - old["min_ms"])
    if old["median_ms"] - new["median_ms"] > spread:
        return "faster"
    if new["median_ms"] - old["median_ms"] > spread:
        return "slower"
    return "within the spread"


def main():
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    ctx = L.init(0)
    rec = dict(rows=ROWS, iters=ITERS, stream_copy_gbs_before=ctx.probe_stream_copy(), products=[], layer=None)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for K in (128, 256):
        x = torch.randn(ROWS, K, device="cuda", generator=gen)
        xb = ctx.cast_f32_bf16(x)
        x = ctx.cast_bf16_f32(xb)  # the same values on both sides
        for N in (128, 256):
            Cf, Cb = torch.zeros(ROWS, N, device="cuda"), torch.zeros(ROWS, N, device="cuda")
            for transB in (False, True):
                B = torch.randn((N, K) if transB else (K, N), device="cuda", generator=gen) * 0.05
                for accum in (False, True):
                    r = alternate(dict(fp32=lambda: ctx.sgemm(x, B, Cf, transB=transB, accum=accum),
                                       bf16=lambda: ctx.gemm_bf16(xb, B, Cb, transB=transB, accum=accum)))
                    by = 2.0 * ROWS * K + 4.0 * ROWS * N * (2 if accum else 1) + 4.0 * K * N
                    row = dict(M=ROWS, N=N, K=K, form="NT" if transB else "NN", accum=accum, **r,
                               bf16_alg_gbs=by / r["bf16"]["median_ms"] / 1e6,
                               bf16_useful_tflops=2.0 * ROWS * N * K / r["bf16"]["median_ms"] / 1e9,
                               bf16_vs_fp32=verdict(r["bf16"], r["fp32"]))
                    print(json.dumps(row), flush=True)
                    rec["products"].append(row)
            del Cf, Cb
        del x, xb
        torch.cuda.empty_cache()
    # the SAGE 256 -> 256 layer step on the products-shaped graph, bf16 tables
    sg = synth.make("ogbn-products", device="cuda", scale=ROWS / 2_449_029)
    g = ctx.graph(sg.rowptr, sg.colidx)
    ctx.sync()
    nv, d = g.nv, 256
    lg = L.LGraph.adopt(g)
    layer = L.Layer(L.SAGE, 1, nv, d, d, lg, True)
    layer.write(L.FEAT_IN, torch.randn(nv, d, device="cuda"))
    layer.write(L.GRAD_IN, torch.randn(nv, d, device="cuda"))
    out, gout = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")
    opt = L.adam(0.01)

    def step(on):
        ctx.set_option("gemm_bf16", on)
        layer.forward(out)
        layer.backward(out, gout)
        layer.update_weight(opt)

    ctx.set_option("agg_bf16", 1)
    try:
        r = alternate(dict(gemm_fp32=lambda: step(0), gemm_bf16=lambda: step(1)))
    finally:
        ctx.set_option("gemm_bf16", 0)
        ctx.set_option("agg_bf16", 0)
    rec["layer"] = dict(layer="sage_256_256", nv=nv, **r, bf16_vs_fp32=verdict(r["gemm_bf16"], r["gemm_fp32"]))
    print(json.dumps(rec["layer"]), flush=True)
    rec["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    L.adam_free(opt)
    layer.close()
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
