"""Hot/cold gathers in the fused, heavy and packed aggregation launches (option spmm_hot_cold) on the products-shaped bench graph
(synth, N = 2 449 029, E = 125.9 M with self loops), swept over the size of the hot set.

Three groups, each with its legs INTERLEAVED in one process (one call of every leg per round, so box and clock state are
shared), timed with HIP events:
  forward   gaib_spmm_gemm as GCN's forward calls it (heavy + fused launch, the aggregate kept, relu), option off and on at
            every hot-set size of --sizes-mb
  backward  gaib_pack_zs + gaib_spmm_gemm_zs as GCN's backward calls them (pack + heavy + fused, the table 50 % kept, the
            aggregate as scratch, W transposed), the same legs
  rows      round 1's leg again: gaib_spmm (the unfused row kernels), spmm_gather_mode 0 against 3 with a 128 MB hot set
Before every timed call of a leg the same call runs untimed -- that is where a changed option rebuilds the graph's flags --
and its output is compared bit for bit with the off leg's.  Per leg: median / min / max and the difference of the medians to
the off leg; `beats_off` is true only where the gain exceeds the larger min-max spread of the two legs.

    python scripts/hotcold_fused.py [--scale 1.0] [--rounds 20] [--sizes-mb 32,64,96,128,160,192,256] [--out PATH]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from graphaibench_amd import capi, layers as L, synth  # noqa: E402


def bits32(t):
    return t.view(torch.int32)


def run_group(ctx, legs, ref_outputs, rounds):
    """legs: {name: (set_options, call, outputs)}; the first leg is the reference (off)"""
    evs = {k: [] for k in legs}
    first = next(iter(legs))
    for r in range(rounds + 2):  # (two warm-up rounds)
        for name, (setup, call, outs) in legs.items():
            setup()
            call()  # untimed: flags rebuilt here when the option changed; the output is checked before the timing
            if name == first:
                for o, ref in zip(outs, ref_outputs):
                    ref.copy_(o)
            else:
                for o, ref in zip(outs, ref_outputs):
                    assert torch.equal(bits32(o), bits32(ref)), f"leg {name} differs from {first} in round {r}"
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            if r >= 2:
                evs[name].append((a, b))
    torch.cuda.synchronize()
    res = {}
    for k, pairs in evs.items():
        ts = sorted(a.elapsed_time(b) for a, b in pairs)
        res[k] = dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1], n=len(ts))
    off = res[first]
    for k, v in res.items():
        if k != first:
            v["gain_ms"] = off["median_ms"] - v["median_ms"]
            v["beats_off"] = bool(v["gain_ms"] > max(off["max_ms"] - off["min_ms"], v["max_ms"] - v["min_ms"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--sizes-mb", default="32,64,96,128,160,192,256")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hotcold" / "hotcold_fused.json"))
    args = ap.parse_args()
    sizes = [int(v) for v in args.sizes_mb.split(",")]
    ctx = L.init(0)
    sg = synth.make("ogbn-products", seed=42, device="cuda", scale=args.scale)
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g = g0.add_selfloop()
    g0.close()
    ctx.sync()
    nv, ne = g.nv, g.ne
    copy0 = ctx.probe_stream_copy()
    rec = dict(graph="ogbn-products synth", nv=nv, ne=ne, rounds=args.rounds, sizes_mb=sizes, stream_copy_gbs_before=copy0,
               graph_stats=ctx.graph_stats(g))
    print(f"nv={nv} ne={ne} stream copy {copy0:.0f} GB/s", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    W = torch.randn(128, 128, device="cuda", generator=gen) * 0.1
    x = torch.randn(nv, 128, device="cuda", generator=gen)
    agg, out = torch.empty(nv, 128, device="cuda"), torch.empty(nv, 128, device="cuda")
    ref_agg, ref_out = torch.empty(nv, 128, device="cuda"), torch.empty(nv, 128, device="cuda")

    def options(hot_cold, mb=None, gather_mode=0):
        def setup():
            ctx.set_option("spmm_gather_mode", gather_mode)
            ctx.set_option("spmm_hot_cold", hot_cold)
            if mb is not None:
                ctx.set_option("spmm_hot_bytes" if gather_mode == 3 else "spmm_hot_cold_bytes", mb << 20)
        return setup

    def counted(call):
        before = ctx.get_option("spmm_hot_cold_launches")
        call()
        return ctx.get_option("spmm_hot_cold_launches") - before

    try:
        # forward
        fwd = lambda: ctx.spmm_gemm(g, capi.W_GCN, x, agg, W, out, relu=True)  # noqa: E731
        legs = {"off": (options(0), fwd, (agg, out))}
        for mb in sizes:
            legs[f"on_{mb}MB"] = (options(1, mb), fwd, (agg, out))
        options(1, sizes[0])()
        assert counted(fwd) == 1, "the forward call did not take the hot/cold form"
        rec["forward"] = run_group(ctx, legs, (ref_agg, ref_out), args.rounds)
        print(json.dumps(dict(forward=rec["forward"])), flush=True)
        # packed backward: the table 50 % kept
        xm = torch.where(torch.rand(nv, 128, device="cuda", generator=gen) < 0.5, x, torch.zeros_like(x))
        zs = torch.empty(nv, 96, dtype=torch.int32, device="cuda")

        def bwd():
            ctx.pack_zs(xm, zs)
            assert ctx.spmm_gemm_zs(g, capi.W_GCN, xm, zs, agg, W, out, transW=True, agg_scratch=True), "refused"

        legs = {"off": (options(0), bwd, (out,))}
        for mb in sizes:
            legs[f"on_{mb}MB"] = (options(1, mb), bwd, (out,))
        options(1, sizes[0])()
        assert counted(bwd) == 1, "the packed call did not take the hot/cold form"
        rec["backward_packed"] = run_group(ctx, legs, (ref_out,), args.rounds)
        print(json.dumps(dict(backward_packed=rec["backward_packed"])), flush=True)
        del zs, xm
        # round 1's leg: the unfused row kernels, gather mode 3 with a 128 MB hot set
        rows = lambda: ctx.spmm(g, capi.W_GCN, x, out)  # noqa: E731
        legs = {"mode_0": (options(0), rows, (out,)), "mode_3_128MB": (options(0, 128, 3), rows, (out,))}
        rec["rows_round1_leg"] = run_group(ctx, legs, (ref_out,), args.rounds)
        print(json.dumps(dict(rows_round1_leg=rec["rows_round1_leg"])), flush=True)
    finally:
        ctx.set_option("spmm_gather_mode", 0)
        ctx.set_option("spmm_hot_bytes", 3 << 20)
        ctx.set_option("spmm_hot_cold", -1)
    rec["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
