"""Zero-suppressed gradient tables on the products-shaped bench graph (synth, N = 2 449 029, E = 125.9 M with self loops).

The backward aggregation of a relu layer gathers a table that is about half +0.0.  This times, with HIP events and the legs of
a group INTERLEAVED (one call of every leg per round, so box and clock state are shared), the dense backward launch set
(gaib_spmm_gemm: heavy + fused) against the packed one (gaib_pack_zs + gaib_spmm_gemm_zs: pack + heavy + fused) on a gradient
masked at a sweep of densities, after checking that both give the same bits.  Per density: median / min / max per leg, the pack
alone, the histogram of values per row and the share of rows over capacity.  `crossover_kept` is the first density of the sweep
at which the packed set is no longer faster than the dense one: the layers' guard stops packing there.
Then the same comparison for the call SAGE's backward makes (MEAN_T weights, the self term as second product), and the values
per row -- in all and per half -- of the gradient the benchmark's own layer step leaves masked (bench.py's graph, seeds, inputs).

    python scripts/zs_aggregation.py [--scale 1.0] [--iters 20] [--densities 0.4,0.5,...] [--out PATH]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from graphaibench_amd import capi, layers as L, synth  # noqa: E402


def interleaved(legs, iters, warmup=3):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in legs}
    for _ in range(iters):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    res = {}
    for k, pairs in evs.items():
        ts = sorted(a.elapsed_time(b) for a, b in pairs)
        res[k] = dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1], n=len(ts))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--densities", default="0.4,0.5,0.6,0.62,0.64,0.66,0.68,0.7,0.8,0.9")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "zs" / "zs_aggregation.json"))
    args = ap.parse_args()
    ctx = L.init(0)
    sg = synth.make("ogbn-products", device="cuda", scale=args.scale)
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g = g0.add_selfloop()
    g0.close()
    ctx.sync()
    nv, ne = g.nv, g.ne
    copy0 = ctx.probe_stream_copy()
    rec = dict(graph="ogbn-products synth", nv=nv, ne=ne, iters=args.iters, stream_copy_gbs_before=copy0, sweep=[])
    print(f"nv={nv} ne={ne} stream copy {copy0:.0f} GB/s", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    W = torch.randn(128, 128, device="cuda", generator=gen) * 0.1
    agg = torch.empty(nv, 128, device="cuda")
    out, out_r = torch.empty(nv, 128, device="cuda"), torch.empty(nv, 128, device="cuda")
    zs = torch.empty(nv, 96, dtype=torch.int32, device="cuda")
    over = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(transW=True, agg_scratch=True)  # the call GCN's backward makes
    for kept in [float(v) for v in args.densities.split(",")]:
        x = torch.randn(nv, 128, device="cuda", generator=gen)
        x = torch.where(torch.rand(nv, 128, device="cuda", generator=gen) < kept, x, torch.zeros_like(x))
        per_row = (x != 0).sum(dim=1)
        hist = torch.bincount(per_row, minlength=129).cpu().tolist()
        over.zero_()
        ctx.pack_zs(x, zs, overflow=over)
        ctx.spmm_gemm(g, capi.W_GCN, x, agg, W, out_r, **kw)
        assert ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out, **kw), "refused"
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), out_r.view(torch.int32)), f"packed aggregation differs at {kept}"
        n_over = int(over.item())
        over_cap = ((x[:, 0::2] != 0).sum(dim=1) > 46) | ((x[:, 1::2] != 0).sum(dim=1) > 46)
        assert n_over == int(over_cap.sum().item())

        def packed_set():
            ctx.pack_zs(x, zs)
            ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out, **kw)

        legs = dict(dense=lambda: ctx.spmm_gemm(g, capi.W_GCN, x, agg, W, out_r, **kw), packed=packed_set,
                    pack_alone=lambda: ctx.pack_zs(x, zs),
                    packed_launches=lambda: ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out, **kw))
        r = dict(kept=kept, bit_identical=True, mean_values_per_row=float(per_row.float().mean().item()),
                 rows_over_capacity=n_over, share_over_capacity=n_over / nv, values_per_row_histogram=hist,
                 legs=interleaved(legs, args.iters))
        d, p = r["legs"]["dense"], r["legs"]["packed"]
        r["gain_ms"] = d["median_ms"] - p["median_ms"]
        r["packed_faster_by_more_than_the_spread"] = bool(r["gain_ms"] > max(d["max_ms"] - d["min_ms"], p["max_ms"] - p["min_ms"]))
        print(json.dumps({k: v for k, v in r.items() if k != "values_per_row_histogram"}), flush=True)
        rec["sweep"].append(r)
        del x
    cross = next((r["kept"] for r in rec["sweep"] if r["gain_ms"] <= 0), None)
    rec["crossover_kept"] = cross
    # the call SAGE's backward makes: transposed-mean weights, the dense rows as the second row operand
    rec["sage_backward_call"] = []
    W2 = torch.randn(128, 128, device="cuda", generator=gen) * 0.1
    for kept in (0.5, 0.6):
        x = torch.randn(nv, 128, device="cuda", generator=gen)
        x = torch.where(torch.rand(nv, 128, device="cuda", generator=gen) < kept, x, torch.zeros_like(x))
        kw2 = dict(transW=True, agg_scratch=True, rows2=x, W2=W2)
        ctx.pack_zs(x, zs)
        ctx.spmm_gemm(g, capi.W_MEAN_T, x, agg, W, out_r, **kw2)
        assert ctx.spmm_gemm_zs(g, capi.W_MEAN_T, x, zs, agg, W, out, **kw2), "refused"
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), out_r.view(torch.int32)), f"packed two-product aggregation differs at {kept}"

        def packed_set2():
            ctx.pack_zs(x, zs)
            ctx.spmm_gemm_zs(g, capi.W_MEAN_T, x, zs, agg, W, out, **kw2)

        legs = dict(dense=lambda: ctx.spmm_gemm(g, capi.W_MEAN_T, x, agg, W, out_r, **kw2), packed=packed_set2)
        r = dict(kept=kept, bit_identical=True, legs=interleaved(legs, args.iters))
        r["gain_ms"] = r["legs"]["dense"]["median_ms"] - r["legs"]["packed"]["median_ms"]
        print(json.dumps(r), flush=True)
        rec["sage_backward_call"].append(r)
        del x
    del agg, out, out_r, zs
    torch.cuda.empty_cache()
    # the benchmark's own masked gradient (bench.py: products graph seed 42, torch seed 43, GCN 128 -> 128 with relu)
    if args.scale == 1.0:
        g.close()
        sg = synth.make("ogbn-products", seed=42, device="cuda", scale=1.0)
        g0 = ctx.graph(sg.rowptr, sg.colidx)
        g1 = g0.add_selfloop()
        g0.close()
        lg = L.LGraph.adopt(g1)
        layer = L.Layer(L.GCN, 1, nv, 128, 128, lg, True, lr=0.01)
        torch.manual_seed(43)
        layer.write(L.FEAT_IN, torch.randn(nv, 128, device="cuda"))
        layer.write(L.GRAD_IN, torch.randn(nv, 128, device="cuda"))
        fo, go = torch.empty(nv, 128, device="cuda"), torch.empty(nv, 128, device="cuda")
        layer.forward(fo)
        layer.backward(fo, go)
        L.sync()
        gm = layer.tensor(L.GRAD_IN, (nv, 128))
        nz = gm.view(torch.int32) != 0
        per_row, ev, od = nz.sum(dim=1), nz[:, 0::2].sum(dim=1), nz[:, 1::2].sum(dim=1)
        rec["bench_gradient"] = dict(
            kept=float(nz.float().mean().item()), mean_values_per_row=float(per_row.float().mean().item()),
            std_values_per_row=float(per_row.float().std().item()), max_values_per_row=int(per_row.max().item()),
            share_rows_over_92=float((per_row > 92).float().mean().item()),
            share_rows_over_46_in_a_half=float(((ev > 46) | (od > 46)).float().mean().item()),
            values_per_row_histogram=torch.bincount(per_row, minlength=129).cpu().tolist(),
            values_per_half_histogram=torch.bincount(torch.cat([ev, od]), minlength=65).cpu().tolist())
        print(json.dumps({k: v for k, v in rec["bench_gradient"].items() if "histogram" not in k}), flush=True)
        layer.close()
    rec["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
