"""Wide zero-suppressed gradient tables (256 columns, one packed image per 128-column K-slab) on the products-shaped graph
(synth, N = 2 449 029, E = 125.9 M with self loops).  One process, HIP events, the legs of a comparison ALTERNATING call by call
(box and clock state shared), median and min-max per leg, the stream-copy rate of the run beside them.

(a) kernel level: the dense backward launch set at 256 -> 256 (gaib_spmm_gemm: two K-slab launches of heavy + fused) against
    gaib_pack_zs_wide + gaib_spmm_gemm_zs, GCN weights, transW, the aggregate as scratch -- the call GCN's backward makes -- on a
    gradient masked at a sweep of kept shares, after checking that both give the same bits; the share of row-slabs over capacity
    is reported with every point, and `guard_crossing_share` is the share at which the gain crosses zero (linear between the two
    sweep points around the sign change): where ZS_GUARD_SHARE (host/aggregators.cpp) should sit at this width.
(b) the GCN and SAGE 256 -> 256 layer steps (forward + backward + Adam) with agg_zs_wide 0 / 1 in alternating pairs.
Reading rule: a leg is faster only if its median wins by more than both legs' spreads (max - min) together.

    python scripts/zs_wide.py [--scale 1.0] [--iters 20] [--kept 0.4,0.5,0.6,0.7] [--out PATH]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from graphaibench_amd import capi, layers as L, synth  # noqa: E402


def alternating(legs, iters, warmup=3):
    for _ in range(warmup):
        for fn in legs.values():
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


def verdict(ref, new):
    """gain of `new` over `ref` and whether it clears the reading rule"""
    gain = ref["median_ms"] - new["median_ms"]
    spreads = (ref["max_ms"] - ref["min_ms"]) + (new["max_ms"] - new["min_ms"])
    return dict(gain_ms=gain, spreads_together_ms=spreads,
                reading="faster" if gain > spreads else ("slower" if -gain > spreads else "no difference beyond the spreads"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kept", default="0.4,0.5,0.6,0.7")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "zs" / "zs_wide.json"))
    args = ap.parse_args()
    ctx = L.init(0)
    sg = synth.make("ogbn-products", device="cuda", scale=args.scale)
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g = g0.add_selfloop()
    g0.close()
    ctx.sync()
    nv, ne = g.nv, g.ne
    copy0 = ctx.probe_stream_copy()
    rec = dict(graph="ogbn-products synth", scale=args.scale, nv=nv, ne=ne, iters=args.iters, stream_copy_gbs_before=copy0,
               reading_rule="a leg is faster only if its median wins by more than both legs' spreads (max - min) together",
               kernel_level=[], layer_steps=[])
    print(f"nv={nv} ne={ne} stream copy {copy0:.0f} GB/s", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(1)

    # ---- (a) the launch sets ----
    W = torch.randn(256, 256, device="cuda", generator=gen) * 0.1
    agg = torch.empty(nv, 256, device="cuda")
    out, out_r = torch.empty(nv, 256, device="cuda"), torch.empty(nv, 256, device="cuda")
    zs = torch.empty(2, nv, 96, dtype=torch.int32, device="cuda")
    over = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(transW=True, agg_scratch=True)
    for kept in [float(v) for v in args.kept.split(",")]:
        x = torch.randn(nv, 256, device="cuda", generator=gen)
        x = torch.where(torch.rand(nv, 256, device="cuda", generator=gen) < kept, x, torch.zeros_like(x))
        over.zero_()
        ctx.pack_zs_wide(x, zs, overflow=over)
        ctx.spmm_gemm(g, capi.W_GCN, x, agg, W, out_r, **kw)
        assert ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out, **kw), "refused"
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), out_r.view(torch.int32)), f"packed aggregation differs at {kept}"
        n_over = int(over.item())

        def packed_set():
            ctx.pack_zs_wide(x, zs)
            ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out, **kw)

        legs = dict(dense=lambda: ctx.spmm_gemm(g, capi.W_GCN, x, agg, W, out_r, **kw), packed=packed_set,
                    pack_alone=lambda: ctx.pack_zs_wide(x, zs),
                    packed_launches=lambda: ctx.spmm_gemm_zs(g, capi.W_GCN, x, zs, agg, W, out, **kw))
        r = dict(kept=kept, bit_identical=True, row_slabs_over_capacity=n_over, share_over_capacity=n_over / (2.0 * nv),
                 legs=alternating(legs, args.iters))
        r.update(verdict(r["legs"]["dense"], r["legs"]["packed"]))
        print(json.dumps(r), flush=True)
        rec["kernel_level"].append(r)
        del x
    cross = None
    pts = rec["kernel_level"]
    for p, q in zip(pts, pts[1:]):
        if p["gain_ms"] > 0 >= q["gain_ms"]:
            t = p["gain_ms"] / (p["gain_ms"] - q["gain_ms"])
            cross = p["share_over_capacity"] + t * (q["share_over_capacity"] - p["share_over_capacity"])
    rec["guard_crossing_share"] = cross
    del agg, out, out_r, zs, W
    torch.cuda.empty_cache()

    # ---- (b) the layer steps ----
    lg = L.LGraph.adopt(g)
    ctx.set_option("agg_zs", 1)
    for kind, name in ((L.GCN, "gcn"), (L.SAGE, "sage")):
        layer = L.Layer(kind, 1, nv, 256, 256, lg, True)
        layer.write(L.FEAT_IN, torch.randn(nv, 256, device="cuda", generator=gen))
        fo, go = torch.empty(nv, 256, device="cuda"), torch.empty(nv, 256, device="cuda")
        opt = L.adam(0.01)
        layer.write(L.GRAD_IN, torch.randn(nv, 256, device="cuda", generator=gen))

        def step_with(on):
            def step():
                ctx.set_option("agg_zs_wide", on)
                layer.forward(fo)
                layer.backward(fo, go)
                layer.update_weight(opt)
            return step

        r = dict(layer=f"{name}_256_256", legs=alternating(dict(agg_zs_wide_0=step_with(0), agg_zs_wide_1=step_with(1)), args.iters))
        r["kept_share_of_the_output"] = float((fo > 0).float().mean().item())
        r["paused_by_the_guard_at_the_end"] = ctx.get_option("agg_zs_paused")
        r.update(verdict(r["legs"]["agg_zs_wide_0"], r["legs"]["agg_zs_wide_1"]))
        print(json.dumps(r), flush=True)
        rec["layer_steps"].append(r)
        ctx.set_option("agg_zs_wide", 0)
        L.adam_free(opt)
        layer.close()
        del fo, go
        torch.cuda.empty_cache()
    rec["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
