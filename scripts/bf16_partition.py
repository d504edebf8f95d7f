"""One rank's partitioned GCN 128 -> 128 step (forward + backward) with fp32 and with bf16 tables, for the build under ROOT --
any checkout of this project: the shard is built by ROOT's own scripts/papers_shard.py (rank 0 of 8; the papers100M-shaped
shard with a uniform or a clustered boundary, or the products strong-scaling share), and every (mode, dtype) leg is timed step
by step here.  A build without bf16 tables on partitions (no LGraph.set_halo_bf16) runs the fp32 legs only: to compare two
builds, run them alternately on one box (parent, new, parent, new), one process each; profiles/bf16/bf16_partition.json is
where the records go.  The all-to-all is replaced by a resident halo table (scripts/papers_shard.py): the pack runs, the wire does not.

    python scripts/bf16_partition.py ROOT OUT.json --leg papers_uniform|papers_clustered|strong [--steps 20] [--scale 1.0]
                                     [--mode split classes onepass auto] [--dtype fp32 bf16]

Per leg: median and min-max of the timed steps after 3 warm-up steps, the dominant kernels' ms per step from gaib_prof_table
(a separate pass of 5 steps with the profiler on), bytes per exchange, the pack time, and whether the owned table is below the
4 GB a buffer descriptor covers.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ap = argparse.ArgumentParser()
ap.add_argument("root")
ap.add_argument("out")
ap.add_argument("--leg", required=True, choices=["papers_uniform", "papers_clustered", "strong"])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--mode", nargs="+", default=["split", "classes", "onepass", "auto"])
ap.add_argument("--dtype", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
args = ap.parse_args()
root = Path(args.root).resolve()
sys.path.insert(0, str(root))
sys.path.insert(0, str(root / "scripts"))
import papers_shard as ps  # noqa: E402  (ROOT's: the shard is cut the same way in both builds)
from graphaibench_amd import capi, layers as L  # noqa: E402

D = ps.D
HAS_BF16 = hasattr(L.LGraph, "set_halo_bf16")
records = []


def one(ctx, mode, S, dtype):
    bf16 = dtype == "bf16"
    eb = 2 if bf16 else 4
    nv, n_halo, send_idx, send_counts, recv_counts = S["nv"], S["n_halo"], S["send_idx"], S["send_counts"], S["recv_counts"]
    g_own = ctx.graph(S["rp_own"], S["ci_own"])
    g_own.set_vertex_norm(S["vd"], S["vd"], S["inv"], row_inv_deg=S["inv"])
    lg = L.LGraph.adopt(g_own)
    g_halo = ctx.graph(S["rp_halo"], S["ci_halo"], ncols=max(n_halo, 1))
    g_halo.set_vertex_norm(S["vd"], S["vd"][S["pick"]], S["inv"][S["pick"]], row_inv_deg=S["inv"])
    lg.set_partition_mode(ps.MODES[mode])
    lg.set_halo_link_rows(max(max(send_counts), max(recv_counts)))
    table = S.setdefault("_table16", S["halo_table"].to(torch.bfloat16)) if bf16 else S["halo_table"]
    sendbuf = torch.empty(max(send_idx.numel(), 1), D, device="cuda", dtype=table.dtype)
    pack_row, pack_slot = torch.sort(send_idx, stable=True)
    pack_slot = pack_slot.contiguous()

    def begin(length, src_ptr):  # the pack of the rows the 7 peers need, in source order as the halo plans do it
        if send_idx.numel():
            capi._check(ctx.lib.gaib_gather_scatter_rows(ctx.h, send_idx.numel(), pack_row.data_ptr(), pack_slot.data_ptr(),
                                                         length * eb // 4, src_ptr, sendbuf.data_ptr()), "gaib_gather_scatter_rows")

    def end(length):
        return table.data_ptr()

    if bf16:
        ctx.set_option("agg_bf16", 1)
        lg.set_halo_bf16(g_halo, begin, end)
    else:
        lg.set_halo(g_halo, begin, end)
    mode_used, n_bnd, _ = lg.partition_mode(D)
    layer = L.Layer(L.GCN, 1, nv, D, D, lg, act=True)
    layer.write(L.FEAT_IN, S["x_in"])
    layer.write(L.GRAD_IN, S["g_in"])
    fo, go = torch.empty(nv, D, device="cuda"), torch.empty(nv, D, device="cuda")

    def step():
        layer.forward(fo)
        layer.backward(fo, go)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    evs = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    ctx.prof_reset()
    ctx.prof_enable(True)
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    ctx.prof_enable(False)
    prof = {k: round(v["ms"] / 5, 3) if isinstance(v, dict) else v for k, v in ctx.prof_table().items()}
    ctx.prof_reset()
    src = S["x_in"].to(torch.bfloat16) if bf16 else S["x_in"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        begin(D, src.data_ptr())
    torch.cuda.synchronize()
    pack_ms = (time.perf_counter() - t0) / 5 * 1e3
    rec = dict(leg=args.leg, mode_asked=mode, mode=L.LGraph.PART_NAMES[mode_used], dtype=dtype, steps=args.steps,
               median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1], n_own=nv, n_halo_rows=n_halo, boundary_rows=n_bnd,
               ne_own_columns=S["ne_own"], ne_halo_columns=S["ne_halo"], send_rows=int(send_idx.numel()),
               send_gb_per_exchange=send_idx.numel() * D * eb / 1e9, recv_gb_per_exchange=n_halo * D * eb / 1e9,
               pack_ms_per_exchange=pack_ms, owned_table_gb=nv * D * eb / 1e9, owned_table_below_4gb=bool(nv * D * eb < 2 ** 32),
               kernels_ms_per_step=prof)
    print(json.dumps(rec), flush=True)
    records.append(rec)
    layer.close()
    lg.close()
    if bf16:
        ctx.set_option("agg_bf16", 0)
    del layer, lg, g_halo, sendbuf, fo, go, src
    torch.cuda.empty_cache()


def timed_mode(ctx, mode, S, steps, pieces=1, **_):
    for dtype in args.dtype:
        if dtype == "bf16" and not HAS_BF16:
            continue
        one(ctx, mode, S, dtype)


ps.run_mode = timed_mode
ctx = L.init(0)
copy_gbs = ctx.probe_stream_copy()
if args.leg == "strong":
    ps.run(ctx, 0, 0.875, args.steps, args.scale, "ogbn-products", "uniform", 0.2, args.mode, "", strong=True)
else:
    ps.run(ctx, 0, 0.1, args.steps, args.scale, "ogbn-papers100M", args.leg.split("_")[1], 0.2, args.mode, "")
Path(args.out).write_text(json.dumps(dict(root=str(root.name), bf16_on_partitions=HAS_BF16, stream_copy_gbs=copy_gbs,
                                          records=records), indent=1) + "\n")
