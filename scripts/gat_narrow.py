"""The one-sweep GAT and GATv2 at rows of 16 and 8 columns (context option gat_fused_narrow) against the staged
path, which is what these widths ran before the option and still run with it off.

Graph: the reddit-shaped graph of bench.py --workload gat-reddit (synth.make("reddit", seed=7), self loops added).  Shapes: 1 head x
16 columns, 2 x 8 (16 columns) and 1 x 8.  Per shape ONE child process under its own `timeout`; inside it the three legs alternate
(iteration i runs all, so drift of the box hits them alike), 20 timed iterations after warm-up, median (min - max) in ms, the
stream-copy rate of the run beside them:
  layer step  GAT layer D -> D, training forward + backward, one layer per leg:
                v1_staged  gat_fused_narrow = 0, gat_v2 = 0   the staged kernels (the behaviour without the option)
                v1_sweep   gat_fused_narrow = 1, gat_v2 = 0   the one-sweep kernels of csrc/gat_narrow.hip
                v2_sweep   gat_fused_narrow = 1, gat_v2 = 1   GATv2 -- another model: what the dynamic score costs beside v1_sweep
  held bytes  device memory each v1 leg's layer holds after its first step (free memory before the layer is built and after)
A shape whose child fails or runs into its time limit ends the run: no further child is started.

    python scripts/gat_narrow.py OUT.json [--iters 20] [--shapes 16x1,16x2,8x1] [--timeout 600]
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

LEGS = dict(v1_staged=dict(gat_fused_narrow=0, gat_v2=0), v1_sweep=dict(gat_fused_narrow=1, gat_v2=0),
            v2_sweep=dict(gat_fused_narrow=1, gat_v2=1))


def child(shape, iters, out_path):
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
    r = dict(len=D, heads=H, nv=nv, ne=ne, iters=iters, legs=LEGS, stream_copy_gbs_before=ctx.probe_stream_copy())
    gen = torch.Generator(device="cuda").manual_seed(1)
    h = torch.randn(nv, D, device="cuda", generator=gen)
    grad = torch.randn(nv, D, device="cuda", generator=gen)
    lout, lgo = torch.empty(nv, D, device="cuda"), torch.empty(nv, D, device="cuda")

    def set_leg(opts):
        for k, v in opts.items():
            ctx.set_option(k, v)

    def free_bytes():
        L.sync()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def make_layer(opts):
        """(layer, its graph, bytes it holds after one training step); the options are set ahead of the layer's construction"""
        set_leg(opts)
        before = free_bytes()
        lg_graph = L.LGraph.adopt(ctx.graph(rp, ci))
        ld = L.Layer(L.GAT, 1, nv, D, D, lg_graph, True)
        ld.set_heads(H)
        ld.write(L.FEAT_IN, h)
        ld.write(L.GRAD_IN, grad)  # (the layer's d_relu masks it in place by the forward output)
        ld.set_phase(0)
        ld.forward(lout)
        ld.backward(lout, lgo)
        return ld, lg_graph, before - free_bytes()

    def step(ld, opts):
        def run():
            set_leg(opts)
            ld.forward(lout)
            ld.backward(lout, lgo)
        return run

    # a throw-away layer per leg first: the context's workspace and the allocator's caches reach their size before anything is measured
    for opts in LEGS.values():
        ld, lgr, _ = make_layer(opts)
        ld.close()
        lgr.close()
    r["held_bytes"] = {}
    for name in ("v1_staged", "v1_sweep"):
        ld, lgr, held = make_layer(LEGS[name])
        r["held_bytes"][name] = held
        ld.close()
        lgr.close()
    made = {name: make_layer(opts) for name, opts in LEGS.items()}
    r["layer_step"] = time_legs({name: step(made[name][0], opts) for name, opts in LEGS.items()}, iters)
    for ld, lgr, _ in made.values():
        ld.close()
        lgr.close()
    set_leg(dict(gat_fused_narrow=0, gat_v2=0))
    g.close()
    r["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    Path(out_path).write_text(json.dumps(r) + "\n")
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="16x1,16x2,8x1")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per shape (its child process)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.iters, args.out)
        return
    rec = dict(what="GAT layer step at rows of 16 and 8 columns: the one-sweep kernels (gat_fused_narrow = 1) beside the staged path "
                    "(0, the behaviour without the option), and GATv2 in one sweep beside the one-sweep GAT",
               graph="reddit synth (seed 7) + self loops", shapes=[])
    with tempfile.TemporaryDirectory() as tmp:
        for shape in args.shapes.split(","):
            part = Path(tmp) / f"{shape}.json"
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, str(Path(__file__).resolve()), str(part), "--child", shape,
                   "--iters", str(args.iters)]
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
