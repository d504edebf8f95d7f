"""The one-sweep GAT forward and backward over bf16 tables against the fp32 sweeps (option gat_bf16).

Graph: the reddit-shaped graph of bench.py --workload gat-reddit (synth.make("reddit", seed=7), self loops added).  Shapes:
8 heads x 8 (len 64), x 4 (len 32), x 16 (len 128).  Legs, interleaved in ONE process (iteration i runs every leg once, so drift
of the box hits all of them alike), 20 timed iterations after warm-up, median (min - max) in ms:
  forward fp32 / bf16; backward fp32 chunk / fp32 packed-math / bf16 chunk / bf16 packed-math (option gat_bwd_pk); the two casts
  (h in forward, grad in backward); the GAT layer step (forward + backward) with gat_bf16 0 and 1; at 8 x 8 also the backward
  sweeps with every gather served by the L2 (column ids >> 5, as scripts/gat_l2_ceiling.py).  The in-run stream-copy rate stands
  beside them.  The packed-table builds run inside the packed-math backward calls and have no entry point of their own:
  --kernels runs the four backward legs at 8 x 8 a few times and exits, for a kernel trace (rocprofv3 --kernel-trace --stats)
  that times the builders and the sweeps kernel by kernel; its figures are merged into the JSON under "kernel_trace".

    python scripts/bf16_gat.py [--iters 20] [--out profiles/bf16/bf16_gat.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bf16_gat.py --kernels
    python scripts/bf16_gat.py --merge-trace DIR/.../*_kernel_stats.csv
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from graphaibench_amd import layers as L, synth  # noqa: E402


def summarise(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def time_legs(legs, iters, warmup=3):
    """legs: {name: callable}; every iteration runs every leg once, each between its own pair of events"""
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
    return {k: summarise([a.elapsed_time(b) for a, b in v]) for k, v in evs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bf16" / "bf16_gat.json"))
    ap.add_argument("--shapes", default="64x8,32x8,128x8")
    ap.add_argument("--kernels", action="store_true", help="the four backward legs at 8 x 8, 5 times each, then exit")
    ap.add_argument("--merge-trace", default=None, help="a rocprofv3 kernel_stats.csv of a --kernels run: merged into --out")
    args = ap.parse_args()
    if args.merge_trace:
        import csv

        rows = [r for r in csv.DictReader(open(args.merge_trace)) if "gat_" in r["Name"] or "rowdot" in r["Name"]]
        rec = json.loads(Path(args.out).read_text())
        rec["kernel_trace"] = [dict(kernel=r["Name"].split("(")[0], calls=int(r["Calls"]), mean_us=float(r["AverageNs"]) / 1e3,
                                    min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3) for r in rows]
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
        return
    ctx = L.init(0)
    sg = synth.make("reddit", seed=7, device="cuda")
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g = g0.add_selfloop()
    g0.close()
    nv, ne = g.nv, g.ne
    rp, ci = g.rowptr(), g.colidx()
    g_l2 = ctx.graph(rp, (ci.to(torch.int64) >> 5).to(torch.int32))  # every gather served by the L2
    ctx.set_option("gat_fused_fwd", 1)
    ctx.set_option("gat_fused_bwd", 1)
    rec = dict(graph="reddit synth (seed 7) + self loops", nv=nv, ne=ne, iters=args.iters,
               stream_copy_gbs_before=ctx.probe_stream_copy(), shapes=[])
    gen = torch.Generator(device="cuda").manual_seed(1)
    for shape in args.shapes.split(","):
        D, H = (int(v) for v in shape.split("x"))
        h = torch.randn(nv, D, device="cuda", generator=gen)
        grad = torch.randn(nv, D, device="cuda", generator=gen)
        al = torch.randn(D, device="cuda", generator=gen) * 0.2
        ar = torch.randn(D, device="cuda", generator=gen) * 0.2
        hb, gb = ctx.cast_f32_bf16(h), ctx.cast_f32_bf16(grad)
        hw, gw = ctx.cast_bf16_f32(hb), ctx.cast_bf16_f32(gb)
        out, stats = torch.empty(nv, D, device="cuda"), torch.empty(nv, H, 2, device="cuda")
        go, lg, rg = torch.empty(nv, D, device="cuda"), torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
        cast_out = torch.empty(nv, D, dtype=torch.bfloat16, device="cuda")
        assert ctx.gat_forward_fused(g, hw, al, ar, out, stats, heads=H)
        fwd = out.clone()

        def bwd32(graph, pk):
            def run():
                ctx.set_option("gat_bwd_pk", pk)
                assert ctx.gat_backward_fused(graph, hw, gw, fwd, al, ar, None, go, lg, rg, heads=H, row_stats=stats)
            return run

        def bwd16(graph, pk):
            def run():
                ctx.set_option("gat_bwd_pk", pk)
                assert ctx.gat_backward_fused_bf16(graph, hb, gb, fwd, al, ar, go, lg, rg, stats, heads=H)
            return run

        legs = {
            "fwd_fp32": lambda: ctx.gat_forward_fused(g, hw, al, ar, out, stats, heads=H),
            "fwd_bf16": lambda: ctx.gat_forward_fused_bf16(g, hb, al, ar, out, stats, heads=H),
            "bwd_fp32_chunk": bwd32(g, 0), "bwd_fp32_pk": bwd32(g, 1), "bwd_bf16_chunk": bwd16(g, 0), "bwd_bf16_pk": bwd16(g, 1),
            "cast_h": lambda: ctx.cast_f32_bf16(h, cast_out), "cast_grad": lambda: ctx.cast_f32_bf16(grad, cast_out),
        }
        if args.kernels:
            for k in ("bwd_fp32_chunk", "bwd_fp32_pk", "bwd_bf16_chunk", "bwd_bf16_pk"):
                for _ in range(5):
                    legs[k]()
            torch.cuda.synchronize()
            return
        if (D, H) == (64, 8):
            legs.update({"bwd_fp32_chunk_l2": bwd32(g_l2, 0), "bwd_bf16_chunk_l2": bwd16(g_l2, 0),
                         "bwd_fp32_pk_l2": bwd32(g_l2, 1), "bwd_bf16_pk_l2": bwd16(g_l2, 1)})
        r = dict(len=D, heads=H, legs=time_legs(legs, args.iters))
        ctx.set_option("gat_bwd_pk", 0)
        r["pairs_table_bytes"] = dict(fp32=nv * (2 * D + 4 * H) * 4, bf16=nv * (D + 4 * H) * 4)
        del hw, gw, out, go, fwd, cast_out
        torch.cuda.empty_cache()

        # the layer step: GAT layer D -> D, H heads, level 1, forward + backward
        lg_graph = L.LGraph.adopt(ctx.graph(rp, ci))
        ld = L.Layer(L.GAT, 1, nv, D, D, lg_graph, True)
        ld.set_heads(H)
        ld.write(L.FEAT_IN, h)
        ld.write(L.GRAD_IN, grad)  # (the layer's d_relu masks it in place by the forward output: stable from step to step)
        lout, lgo = torch.empty(nv, D, device="cuda"), torch.empty(nv, D, device="cuda")

        def step(on):
            def run():
                ctx.set_option("gat_bf16", on)
                ld.forward(lout)
                ld.backward(lout, lgo)
            return run

        r["layer_step"] = time_legs({"gat_bf16_0": step(0), "gat_bf16_1": step(1)}, args.iters)
        ctx.set_option("gat_bf16", 0)
        ld.close()
        lg_graph.close()
        del h, grad, hb, gb, lout, lgo
        torch.cuda.empty_cache()
        print(json.dumps(r), flush=True)
        rec["shapes"].append(r)
    rec["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
