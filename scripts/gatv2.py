"""The one-sweep GATv2 (context option gat_v2) next to the one-sweep GAT of the same tree.

Graph: the reddit-shaped graph of bench.py --workload gat-reddit (synth.make("reddit", seed=7), self loops added).  Shapes: 8 heads
x 8 columns and 1 head x 64.  Per shape ONE child process under its own `timeout`; inside it the two legs alternate (iteration i
runs both, so drift of the box hits them alike), 20 timed iterations after warm-up, median (min - max) in ms, the stream-copy
rate of the run beside them:
  layer step  GAT layer D -> D, training forward + backward, one layer per leg: gat_v2_0 (the v1 one-sweep kernels) and gat_v2_1
  calls       the forward and the backward call alone: gaib_gat_forward_fused / gaib_gat_backward_fused (row statistics) and
              gaib_gatv2_forward / gaib_gatv2_backward on the same tables
The two legs compute different models: the comparison says what the dynamic score costs, not which path to take.
Rows wider than 128 columns (256x1, 512x1, 256x8 = 8 heads x 32: DESIGN.md 3.3.6) run both legs on their opt-in one-sweep paths:
gat_fused_head = gat_fused_wide = 1 for the static scores, gatv2_wide = 1 for GATv2, set for the whole child and recorded.
--drop RATE: both legs under attention dropout kept in the sweep -- gat_fused_drop = 1 and layers with score_drop
= RATE, the calls alone through gaib_gat_*_fused_drop and gaib_gatv2_*_drop under one seed.  Not measured yet.
--dtype bf16: BOTH legs are GATv2, on fp32 tables (gat_v2 = 1, gat_bf16 = 0) and on bf16 tables (gat_v2 = gat_bf16 =
1: the layer casts h and the incoming gradient, inside the timed step); the calls alone are gaib_gatv2_* and gaib_gatv2_*_bf16 on h,
grad and their bf16 casts made once.  Composes with --shapes and --drop.  Not measured yet.
A shape whose child fails or runs into its time limit ends the run: no further child is started.

    python scripts/gatv2.py OUT.json [--iters 20] [--shapes 64x8,64x1] [--timeout 600]
    python scripts/gatv2.py OUT.json --shapes 256x1,512x1,256x8
    python scripts/gatv2.py OUT.json --shapes 64x8,256x1,256x8 --drop 0.3
    python scripts/gatv2.py OUT.json --shapes 64x8,64x1,256x8,256x1 --dtype bf16
"""
import argparse
import json
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))


def child(shape, iters, out_path, drop=0.0, dtype="fp32"):
    import torch

    from bf16_gat import time_legs
    from graphaibench_amd import layers as L, synth

    ctx = L.init(0)
    sg = synth.make("reddit", seed=7, device="cuda")
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g = g0.add_selfloop()
    g0.close()
    nv, ne = g.nv, g.ne
    rp, ci = g.rowptr(), g.colidx()
    D, H = (int(v) for v in shape.split("x"))
    r = dict(len=D, heads=H, nv=nv, ne=ne, iters=iters, drop=drop, dtype=dtype, stream_copy_gbs_before=ctx.probe_stream_copy())
    r["options"] = {}
    if D > 128:  # the wide rows' one-sweep paths of both models, before a layer is built
        r["options"].update(gat_fused_head=1, gat_fused_wide=1, gatv2_wide=1)
    if drop > 0:  # attention dropout stays in the sweeps of both models
        r["options"].update(gat_fused_drop=1)
    for k, v in r["options"].items():
        ctx.set_option(k, v)
    gen = torch.Generator(device="cuda").manual_seed(1)
    h = torch.randn(nv, D, device="cuda", generator=gen)
    grad = torch.randn(nv, D, device="cuda", generator=gen)
    lout, lgo = torch.empty(nv, D, device="cuda"), torch.empty(nv, D, device="cuda")

    # a leg of the layer step: the options set ahead of its layer's construction and of each of its steps
    legs = dict(gat_v2_0=dict(gat_v2=0), gat_v2_1=dict(gat_v2=1))
    if dtype == "bf16":
        legs = dict(v2_fp32=dict(gat_v2=1, gat_bf16=0), v2_bf16=dict(gat_v2=1, gat_bf16=1))

    def set_leg(opts):
        for k, v in opts.items():
            ctx.set_option(k, v)

    def make_layer(opts):
        set_leg(opts)
        lg_graph = L.LGraph.adopt(ctx.graph(rp, ci))
        ld = L.Layer(L.GAT, 1, nv, D, D, lg_graph, True, score_drop=drop)
        ld.set_heads(H)
        ld.write(L.FEAT_IN, h)
        ld.write(L.GRAD_IN, grad)  # (the layer's d_relu masks it in place by the forward output)
        ld.set_phase(0)
        return ld, lg_graph

    def step(ld, opts):
        def run():
            set_leg(opts)
            ld.forward(lout)
            ld.backward(lout, lgo)
        return run

    made = {name: (make_layer(opts), opts) for name, opts in legs.items()}
    r["layer_step"] = time_legs({name: step(ld, opts) for name, ((ld, _), opts) in made.items()}, iters)
    for (ld, lgr), _ in made.values():
        ld.close()
        lgr.close()
    set_leg(dict(gat_v2=0, gat_bf16=0))
    al, ar = (0.05 * torch.randn(D, device="cuda", generator=gen) for _ in range(2))
    stats, lg_, rg_ = torch.empty(nv, H, 2, device="cuda"), torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    ok = lambda done: done or sys.exit("a call was refused")  # noqa: E731
    seed = 0x5EED0001
    if dtype == "bf16":
        hb, gb = ctx.cast_f32_bf16(h), ctx.cast_f32_bf16(grad)
    r["calls"] = time_legs({
        "v2_forward_fp32": lambda: ok(ctx.gatv2_forward_drop(g, h, al, lout, stats, drop, seed, heads=H)),
        "v2_forward_bf16": lambda: ok(ctx.gatv2_forward_drop_bf16(g, hb, al, lout, stats, drop, seed, heads=H)),
        "v2_backward_fp32": lambda: ok(ctx.gatv2_backward_drop(g, h, grad, lout, al, stats, lgo, lg_, drop, seed, heads=H)),
        "v2_backward_bf16": lambda: ok(ctx.gatv2_backward_drop_bf16(g, hb, gb, lout, al, stats, lgo, lg_, drop, seed, heads=H)),
    } if dtype == "bf16" and drop > 0 else {
        "v2_forward_fp32": lambda: ok(ctx.gatv2_forward(g, h, al, lout, stats, heads=H)),
        "v2_forward_bf16": lambda: ok(ctx.gatv2_forward_bf16(g, hb, al, lout, stats, heads=H)),
        "v2_backward_fp32": lambda: ok(ctx.gatv2_backward(g, h, grad, lout, al, stats, lgo, lg_, heads=H)),
        "v2_backward_bf16": lambda: ok(ctx.gatv2_backward_bf16(g, hb, gb, lout, al, stats, lgo, lg_, heads=H)),
    } if dtype == "bf16" else {
        "v1_forward": lambda: ok(ctx.gat_forward_fused_drop(g, h, al, ar, lout, stats, drop, seed, heads=H)),
        "v2_forward": lambda: ok(ctx.gatv2_forward_drop(g, h, al, lout, stats, drop, seed, heads=H)),
        "v1_backward": lambda: ok(ctx.gat_backward_fused_drop(g, h, grad, lout, al, ar, lgo, lg_, rg_, stats, drop, seed, heads=H)),
        "v2_backward": lambda: ok(ctx.gatv2_backward_drop(g, h, grad, lout, al, stats, lgo, lg_, drop, seed, heads=H)),
    } if drop > 0 else {
        "v1_forward": lambda: ok(ctx.gat_forward_fused(g, h, al, ar, lout, stats, heads=H)),
        "v2_forward": lambda: ok(ctx.gatv2_forward(g, h, al, lout, stats, heads=H)),
        "v1_backward": lambda: ok(ctx.gat_backward_fused(g, h, grad, lout, al, ar, None, lgo, lg_, rg_, heads=H, row_stats=stats)),
        "v2_backward": lambda: ok(ctx.gatv2_backward(g, h, grad, lout, al, stats, lgo, lg_, heads=H)),
    }, iters)
    g.close()
    r["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    Path(out_path).write_text(json.dumps(r) + "\n")
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="64x8,64x1")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per shape (its child process)")
    ap.add_argument("--drop", type=float, default=0.0, help="attention dropout rate of both legs, kept in the sweeps (0: none)")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32", help="bf16: both legs GATv2, on fp32 and on bf16 tables")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.iters, args.out, args.drop, args.dtype)
        return
    rec = dict(what="GAT layer step and the two calls alone: GATv2 scores in one sweep (gat_v2 = 1) next to the one-sweep GAT "
                    "(gat_v2 = 0) of the same tree", graph="reddit synth (seed 7) + self loops", shapes=[])
    if args.dtype == "bf16":
        rec["what"] = ("GAT layer step and the two calls alone under GATv2 scores (gat_v2 = 1): fp32 tables next to bf16 tables "
                       "(gat_bf16 = 1) of the same tree")
    with tempfile.TemporaryDirectory() as tmp:
        for shape in args.shapes.split(","):
            part = Path(tmp) / f"{shape}.json"
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, str(Path(__file__).resolve()), str(part), "--child", shape,
                   "--iters", str(args.iters), "--drop", str(args.drop), "--dtype", args.dtype]
            rc = subprocess.run(cmd).returncode
            if rc != 0:  # a fault, an abort or the time limit: nothing more is started on the device
                rec["stopped"] = dict(shape=shape, exit_status=rc)
                break
            rec["shapes"].append(json.loads(part.read_text()))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    sys.exit(1 if "stopped" in rec else 0)


if __name__ == "__main__":
    main()
