"""GCN / SAGE layer steps (forward + backward + Adam) at 128 -> 128 and 256 -> 256 on the products-shaped graph, fp32 tables and
bf16 tables (context option agg_bf16), for the build under ROOT -- any checkout of this project that has the option.  One
build per process: to compare two builds, run them alternately on one box (parent, new, parent, new), as the
"alternation_with_parent_build" section of profiles/bf16/bf16_fused.json was taken.  20 timed steps after 3 warm-up steps
per leg; median, min, max and the in-run stream-copy rate.

    python scripts/bf16_layer_steps.py ROOT OUT.json
"""
import json
import sys
from pathlib import Path
import torch
root = Path(sys.argv[1]).resolve()
sys.path.insert(0, str(root))
from graphaibench_amd import capi, layers as L, synth  # noqa: E402

ctx = L.init(0)
sg = synth.make("ogbn-products", device="cuda", scale=1.0)
g0 = ctx.graph(sg.rowptr, sg.colidx)
g = g0.add_selfloop()
g0.close()
ctx.sync()
nv = g.nv
rec = dict(stream_copy_gbs=ctx.probe_stream_copy(), layers=[])
lg = L.LGraph.adopt(g)
for d in (128, 256):
    for kind, name in ((L.GCN, "gcn"), (L.SAGE, "sage")):
        layer = L.Layer(kind, 1, nv, d, d, lg, True)
        layer.write(L.FEAT_IN, torch.randn(nv, d, device="cuda"))
        out, gout = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")
        opt = L.adam(0.01)
        layer.write(L.GRAD_IN, torch.randn(nv, d, device="cuda"))

        def step():
            layer.forward(out)
            layer.backward(out, gout)
            layer.update_weight(opt)

        r = dict(layer=f"{name}_{d}_{d}")
        for on in (0, 1):
            ctx.set_option("agg_bf16", on)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            evs = []
            for _ in range(20):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step()
                b.record()
                evs.append((a, b))
            torch.cuda.synchronize()
            ts = sorted(a.elapsed_time(b) for a, b in evs)
            r["bf16" if on else "fp32"] = dict(median_ms=ts[10], min_ms=ts[0], max_ms=ts[-1], n=20)
        ctx.set_option("agg_bf16", 0)
        print(json.dumps(r), flush=True)
        rec["layers"].append(r)
        L.adam_free(opt)
        layer.close()
        del out, gout
        torch.cuda.empty_cache()
Path(sys.argv[2]).write_text(json.dumps(rec, indent=1) + "\n")
