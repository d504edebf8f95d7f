"""bf16 feature tables on the products-shaped bench graph (synth, N = 2 449 029, E = 125.9 M with self loops).

First checks that gaib_spmm_bf16 is bit-identical to gaib_spmm_ex on the widened table at every width, then times with
HIP events: gaib_spmm (fp32 table) against gaib_spmm_bf16 and its lane layouts, the cast, and a GCN 128 -> 128 and a
SAGE 128 layer step (forward + backward + update) with the context option agg_bf16 off and on.  Algorithmic bytes count
2 B per gathered bf16 element.  Writes one JSON record (default profiles/bf16/bf16_aggregation.json).

    python scripts/bf16_aggregation.py [--scale 1.0] [--iters 5] [--out PATH]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from graphaibench_amd import capi, layers as L, synth  # noqa: E402


def timeit(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bf16" / "bf16_aggregation.json"))
    args = ap.parse_args()
    ctx = L.init(0)  # the layer library's context: the layer steps below run on it too
    sg = synth.make("ogbn-products", device="cuda", scale=args.scale)
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g = g0.add_selfloop()
    g0.close()
    ctx.sync()
    nv, ne = g.nv, g.ne
    copy_gbs = ctx.probe_stream_copy()
    rec = dict(graph="ogbn-products synth", nv=nv, ne=ne, stream_copy_gbs=copy_gbs, spmm=[], layers=[])
    print(f"nv={nv} ne={ne} stream copy {copy_gbs:.0f} GB/s", flush=True)

    def frac(nbytes, ms):
        gbs = nbytes / ms / 1e6
        return dict(alg_gbs=gbs, frac_8tbs=gbs / 8000, frac_copy=gbs / copy_gbs)

    for d in (47, 100, 128, 256):
        x = torch.randn(nv, d, device="cuda")
        xb = ctx.cast_f32_bf16(x)
        xw = ctx.cast_bf16_f32(xb)
        out, ref = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")
        ctx.spmm(g, capi.W_GCN, xw, ref)
        ctx.spmm_bf16(g, capi.W_GCN, xb, out)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), f"bf16 aggregation differs from fp32 at {d}"
        b32 = ne * (4.0 * d + 8) + nv * 4.0 * d + (nv + 1) * 8.0  # gathered row + col id + weight, output, row pointers
        b16 = ne * (2.0 * d + 8) + nv * 4.0 * d + (nv + 1) * 8.0
        r = dict(d=d, bit_identical=True)
        r["fp32_ms"] = timeit(lambda: ctx.spmm(g, capi.W_GCN, x, ref), args.iters)
        r["fp32"] = frac(b32, r["fp32_ms"])
        for layout in (0, 4, 8):
            if layout and (d % layout or d > 32 * layout):
                continue
            ctx.set_option("spmm_bf16_layout", layout)
            ms = timeit(lambda: ctx.spmm_bf16(g, capi.W_GCN, xb, out), args.iters)
            r[f"bf16_layout{layout}_ms"] = ms
            r[f"bf16_layout{layout}"] = frac(b16, ms)
        ctx.set_option("spmm_bf16_layout", 0)
        r["bf16_ms"] = r["bf16_layout0_ms"]
        r["cast_ms"] = timeit(lambda: ctx.cast_f32_bf16(x, xb), args.iters)
        r["cast"] = frac(6.0 * nv * d, r["cast_ms"])
        print(json.dumps(r), flush=True)
        rec["spmm"].append(r)
        del x, xb, xw, out, ref
        torch.cuda.empty_cache()

    lg = L.LGraph.adopt(g)
    for kind, name in ((L.GCN, "gcn_128_128"), (L.SAGE, "sage_128_128")):
        layer = L.Layer(kind, 1, nv, 128, 128, lg, True)
        layer.write(L.FEAT_IN, torch.randn(nv, 128, device="cuda"))
        gin = torch.randn(nv, 128, device="cuda")
        out, gout = torch.empty(nv, 128, device="cuda"), torch.empty(nv, 128, device="cuda")
        opt = L.adam(0.01)

        layer.write(L.GRAD_IN, gin)

        def step():
            layer.forward(out)
            layer.backward(out, gout)
            layer.update_weight(opt)

        r = dict(layer=name)
        for on in (0, 1):
            ctx.set_option("agg_bf16", on)
            t0 = time.perf_counter()
            r[("bf16" if on else "fp32") + "_step_ms"] = timeit(step, args.iters)
            r[("bf16" if on else "fp32") + "_wall_s"] = time.perf_counter() - t0
        ctx.set_option("agg_bf16", 0)
        print(json.dumps(r), flush=True)
        rec["layers"].append(r)
        L.adam_free(opt)
        layer.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
