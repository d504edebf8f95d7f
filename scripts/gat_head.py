"""The one-sweep GAT for ONE head of 256 or 512 columns (option gat_fused_head) against the staged path.

Graph: the reddit-shaped graph of bench.py --workload gat-reddit (synth.make("reddit", seed=7), self loops added).  Shapes:
1 head x 256 and 1 head x 512.  Per shape ONE child process under its own `timeout`; inside it option 0 and option 1 alternate
(iteration i runs both legs once, so drift of the box hits them alike), 20 timed iterations after warm-up, median (min - max) in
ms, the stream-copy rate of the run beside them:
  layer step  GAT layer D -> D with one head, no attention dropout, training forward + backward, one layer per setting
  memory      device memory each setting holds after its first step: free memory before the layer is built and after the step
              (as tests/test_gpu_lifecycle.py measures it), one layer per setting, built and released in turn
A shape whose child fails or runs into its time limit ends the run: no further child is started.

    python scripts/gat_head.py OUT.json [--iters 20] [--shapes 256x1,512x1] [--timeout 600]
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


def child(shape, iters, out_path):
    import torch

    from bf16_gat import time_legs
    from graphaibench_amd import capi, layers as L, synth

    ctx = L.init(0)
    sg = synth.make("reddit", seed=7, device="cuda")
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g = g0.add_selfloop()
    g0.close()
    nv, ne = g.nv, g.ne
    rp, ci = g.rowptr(), g.colidx()
    g.close()
    D, H = (int(v) for v in shape.split("x"))
    cpl = capi.gat_fused_head_cpl(D, H)
    assert cpl > 0, (D, H)
    r = dict(len=D, heads=H, columns_per_lane=cpl, nv=nv, ne=ne, iters=iters, stream_copy_gbs_before=ctx.probe_stream_copy())
    gen = torch.Generator(device="cuda").manual_seed(1)
    h = torch.randn(nv, D, device="cuda", generator=gen)
    grad = torch.randn(nv, D, device="cuda", generator=gen)
    lout, lgo = torch.empty(nv, D, device="cuda"), torch.empty(nv, D, device="cuda")

    def free_bytes():
        L.sync()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def make_layer(option):
        """(layer, its graph, bytes it holds after one training step)"""
        ctx.set_option("gat_fused_head", option)
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

    def step(ld, option):
        def run():
            ctx.set_option("gat_fused_head", option)
            ld.forward(lout)
            ld.backward(lout, lgo)
        return run

    # a throw-away layer first: the context's workspace and the allocator's caches reach their size before anything is measured
    ld, lgr, _ = make_layer(0)
    ld.close()
    lgr.close()
    r["held_bytes"] = {}
    for option in (0, 1):
        ld, lgr, held = make_layer(option)
        r["held_bytes"][f"gat_fused_head_{option}"] = held
        ld.close()
        lgr.close()
    l0, g0_, _ = make_layer(0)
    l1, g1_, _ = make_layer(1)
    r["layer_step"] = time_legs({"gat_fused_head_0": step(l0, 0), "gat_fused_head_1": step(l1, 1)}, iters)
    ctx.set_option("gat_fused_head", 0)
    for x in (l0, l1, g0_, g1_):
        x.close()
    r["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    Path(out_path).write_text(json.dumps(r) + "\n")
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="256x1,512x1")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per shape (its child process)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.iters, args.out)
        return
    rec = dict(what="GAT layer with ONE head of 256 / 512 columns: one-sweep kernels with the wave on one edge (gat_fused_head = 1) "
                    "against the staged path (0, the baseline)", graph="reddit synth (seed 7) + self loops", shapes=[])
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
