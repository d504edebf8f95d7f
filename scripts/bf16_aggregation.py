"""bf16 feature tables on the products-shaped bench graph (synth, N = 2 449 029, E = 125.9 M with self loops).

First checks that gaib_spmm_bf16 is bit-identical to gaib_spmm_ex on the widened table at every width, then times with
HIP events: gaib_spmm (fp32 table) against gaib_spmm_bf16 and its lane layouts, the cast, and a GCN 128 -> 128 and a
SAGE 128 layer step (forward + backward + update) with the context option agg_bf16 off and on.  Algorithmic bytes count
2 B per gathered bf16 element.  Writes one JSON record (default profiles/bf16/bf16_aggregation.json).

    python scripts/bf16_aggregation.py [--scale 1.0] [--iters 5] [--out PATH]

--fused: the fused aggregation + product over a bf16 table instead (default record profiles/bf16/bf16_fused.json).  After a
bit check against gaib_spmm_gemm on the widened table, the legs of one group are timed INTERLEAVED -- one call of every leg per
round, --iters rounds (at least 20) after warm-up -- so that box and clock state are shared; median, min and max per leg and
the stream-copy rate before and after.  Groups: the call alone at 128 -> 128 and 256 -> 256 with the aggregate kept and as
scratch (gaib_spmm_gemm_bf16 | the two-kernel route gaib_spmm_bf16 + gaib_sgemm_ex, which is that entry point under
spmm_fuse = 0 | fp32 gaib_spmm_gemm), the gathers in flight of the headline variant (spmm_bf16_fuse_u = 16 | 32), and the GCN
and SAGE layer steps at 128 and 256 (fp32 | bf16 tables | bf16 tables under spmm_fuse = 0: the route before the fused kernel
had a bf16 form).

    python scripts/bf16_aggregation.py --fused [--scale 1.0] [--iters 20] [--out PATH]

--strided: odd-width bf16 tables at a line-aligned row stride (default record profiles/bf16/bf16_strided.json).  At 47 and 100
columns, GCN weights: after a bit check of gaib_spmm_bf16_ld against gaib_spmm_bf16, the dense-stride leg (gaib_cast_f32_bf16 +
gaib_spmm_bf16) against the padded one (gaib_cast_f32_bf16_rows to 64 / 128 elements + gaib_spmm_bf16_ld), INTERLEAVED as above,
--iters rounds (at least 20) after warm-up; the gathers alone and the two casts alone the same way; median, min and max per
leg, the stream-copy rate before and after.  `gate`: the padded leg's median below the dense one's by more than the two
legs' min-max spreads together -- what gaib_bf16_row_stride's rule has to meet at a width to keep its stride there.

    python scripts/bf16_aggregation.py --strided [--scale 1.0] [--iters 20] [--out PATH]
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


def interleaved(legs, iters, warmup=3):
    """legs: {name: (setup, fn)} -- setup() (options; not timed) then fn() between an event pair, one leg after the other,
    `iters` rounds.  Returns {name: dict(median_ms, min_ms, max_ms, n)}."""
    for setup, fn in legs.values():
        setup()
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in legs}
    for _ in range(iters):
        for k, (setup, fn) in legs.items():
            setup()
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


def fused_main(args):
    iters = max(args.iters, 20)
    ctx = L.init(0)
    sg = synth.make("ogbn-products", device="cuda", scale=args.scale)
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g = g0.add_selfloop()
    g0.close()
    ctx.sync()
    nv, ne = g.nv, g.ne
    copy0 = ctx.probe_stream_copy()
    rec = dict(graph="ogbn-products synth", nv=nv, ne=ne, iters=iters, stream_copy_gbs_before=copy0, calls=[], fuse_u=[], layers=[])
    print(f"nv={nv} ne={ne} stream copy {copy0:.0f} GB/s", flush=True)

    def opts(**kw):
        def setup():
            for k, v in kw.items():
                ctx.set_option(k, v)
        return setup

    try:
        for d in (128, 256):
            x = torch.randn(nv, d, device="cuda")
            xb = ctx.cast_f32_bf16(x)
            xw = ctx.cast_bf16_f32(xb)
            W = torch.randn(d, d, device="cuda") * 0.1
            agg, out = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")
            agg_r, out_r = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")
            ctx.spmm_gemm(g, capi.W_GCN, xw, agg_r, W, out_r)
            ctx.spmm_gemm_bf16(g, capi.W_GCN, xb, agg, W, out)
            torch.cuda.synchronize()
            same = torch.equal(out.view(torch.int32), out_r.view(torch.int32)) and torch.equal(agg.view(torch.int32), agg_r.view(torch.int32))
            assert same, f"fused bf16 call differs from the fp32 call on the widened table at {d}"
            del xw, agg_r, out_r
            torch.cuda.empty_cache()
            on, off = opts(spmm_fuse=1, spmm_bf16_fuse_u=0), opts(spmm_fuse=0, spmm_bf16_fuse_u=0)
            legs = {}
            for keep in (True, False):
                kw = dict(agg_scratch=not keep)
                tag = "keep" if keep else "scratch"
                legs[f"bf16_fused_{tag}"] = (on, lambda kw=kw: ctx.spmm_gemm_bf16(g, capi.W_GCN, xb, agg, W, out, **kw))
                legs[f"bf16_two_kernel_{tag}"] = (off, lambda kw=kw: ctx.spmm_gemm_bf16(g, capi.W_GCN, xb, agg, W, out, **kw))
                legs[f"fp32_fused_{tag}"] = (on, lambda kw=kw: ctx.spmm_gemm(g, capi.W_GCN, x, agg, W, out, **kw))
            r = dict(d=d, kind="W_GCN", bit_identical=True, legs=interleaved(legs, iters))
            print(json.dumps(r), flush=True)
            rec["calls"].append(r)
            if d == 128:  # gathers in flight of the headline variant (row form, 8-row strip, buffer addressing, 8-B lanes)
                for kind, kname in ((capi.W_MEAN, "W_MEAN"), (capi.W_GCN, "W_GCN")):
                    legs = {f"u{u}": (opts(spmm_fuse=1, spmm_bf16_fuse_u=u),
                                      lambda kind=kind: ctx.spmm_gemm_bf16(g, kind, xb, agg, W, out)) for u in (16, 32)}
                    r = dict(d=d, kind=kname, legs=interleaved(legs, iters))
                    print(json.dumps(r), flush=True)
                    rec["fuse_u"].append(r)
            del x, xb, W, agg, out
            torch.cuda.empty_cache()

        ctx.set_option("spmm_bf16_fuse_u", 0)
        lg = L.LGraph.adopt(g)
        for d in (128, 256):
            for kind, name in ((L.GCN, "gcn"), (L.SAGE, "sage")):
                layer = L.Layer(kind, 1, nv, d, d, lg, True)
                layer.write(L.FEAT_IN, torch.randn(nv, d, device="cuda"))
                gin = torch.randn(nv, d, device="cuda")
                out, gout = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")
                opt = L.adam(0.01)
                layer.write(L.GRAD_IN, gin)

                def step():
                    layer.forward(out)
                    layer.backward(out, gout)
                    layer.update_weight(opt)

                legs = dict(fp32=(opts(agg_bf16=0, spmm_fuse=1), step), bf16_fused=(opts(agg_bf16=1, spmm_fuse=1), step),
                            bf16_two_kernel=(opts(agg_bf16=1, spmm_fuse=0), step))
                r = dict(layer=f"{name}_{d}_{d}", legs=interleaved(legs, iters))
                b, f = r["legs"]["bf16_two_kernel"], r["legs"]["bf16_fused"]
                r["gate_fused_below_baseline_by_more_than_its_spread"] = bool(b["median_ms"] - f["median_ms"] > b["max_ms"] - b["min_ms"])
                print(json.dumps(r), flush=True)
                rec["layers"].append(r)
                L.adam_free(opt)
                layer.close()
                del gin, out, gout
                torch.cuda.empty_cache()
    finally:
        for k, v in dict(agg_bf16=0, spmm_fuse=1, spmm_bf16_fuse_u=0).items():
            ctx.set_option(k, v)
    rec["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    out_path = Path(args.out) if args.out else ROOT / "profiles" / "bf16" / "bf16_fused.json"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote", out_path)


def strided_main(args):
    iters = max(args.iters, 20)
    ctx = L.init(0)
    sg = synth.make("ogbn-products", device="cuda", scale=args.scale)
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g = g0.add_selfloop()
    g0.close()
    ctx.sync()
    nv, ne = g.nv, g.ne
    copy0 = ctx.probe_stream_copy()
    rec = dict(graph="ogbn-products synth", nv=nv, ne=ne, iters=iters, stream_copy_gbs_before=copy0, widths=[])
    print(f"nv={nv} ne={ne} stream copy {copy0:.0f} GB/s", flush=True)
    none = lambda: None
    for d in (47, 100):
        ld = ((2 * d + 63) // 64 * 64) // 2  # the row bytes rounded up to 64: the rule's candidate, whatever the rule says today
        x = torch.randn(nv, d, device="cuda")
        xb = torch.empty(nv, d, dtype=torch.bfloat16, device="cuda")
        xs = torch.empty(nv, ld, dtype=torch.bfloat16, device="cuda")
        out, ref = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")
        ctx.cast_f32_bf16(x, xb)
        ctx.cast_f32_bf16_rows(x, ld, xs)
        ctx.spmm_bf16(g, capi.W_GCN, xb, ref)
        ctx.spmm_bf16(g, capi.W_GCN, xs, out, ld=ld)
        torch.cuda.synchronize()
        assert torch.equal(xs[:, :d].contiguous().view(torch.int16), xb.view(torch.int16)) and not bool(xs[:, d:].view(torch.int16).any())
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), f"strided bf16 aggregation differs from the dense one at {d}"
        del ref
        cast_d, cast_p = (lambda: ctx.cast_f32_bf16(x, xb)), (lambda: ctx.cast_f32_bf16_rows(x, ld, xs))
        gather_d = lambda: ctx.spmm_bf16(g, capi.W_GCN, xb, out)
        gather_p = lambda: ctx.spmm_bf16(g, capi.W_GCN, xs, out, ld=ld)
        r = dict(d=d, ld=ld, rule_ld=ctx.bf16_row_stride(g, d), kind="W_GCN", bit_identical=True)
        r["cast_and_gather"] = interleaved(dict(dense=(none, lambda: (cast_d(), gather_d())), padded=(none, lambda: (cast_p(), gather_p()))), iters)
        r["gather"] = interleaved(dict(dense=(none, gather_d), padded=(none, gather_p)), iters)
        r["cast"] = interleaved(dict(dense=(none, cast_d), padded=(none, cast_p)), iters)
        a, b = r["cast_and_gather"]["dense"], r["cast_and_gather"]["padded"]
        r["gate"] = bool(a["median_ms"] - b["median_ms"] > (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"]))
        b16 = ne * (2.0 * d + 8) + nv * 4.0 * d + (nv + 1) * 8.0  # algorithmic: 2 d bytes per gathered row at either stride
        for k in ("dense", "padded"):
            r["gather"][k]["frac_8tbs"] = b16 / r["gather"][k]["median_ms"] / 1e6 / 8000
        print(json.dumps(r), flush=True)
        rec["widths"].append(r)
        del x, xb, xs, out
        torch.cuda.empty_cache()
    rec["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    out_path = Path(args.out) if args.out else ROOT / "profiles" / "bf16" / "bf16_strided.json"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fused", action="store_true", help="the fused aggregation + product over a bf16 table (see above)")
    ap.add_argument("--strided", action="store_true", help="odd-width bf16 tables at a line-aligned row stride (see above)")
    args = ap.parse_args()
    if args.fused:
        return fused_main(args)
    if args.strided:
        return strided_main(args)
    if args.out is None:
        args.out = str(ROOT / "profiles" / "bf16" / "bf16_aggregation.json")
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
