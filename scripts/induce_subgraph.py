"""Sampled training subgraphs built on the host against built on the device (option sampler_device).

What is timed is everything the trainer's subgraph_sampling() does per epoch AFTER vertex selection, through the hook
gaibl_sampling_build (host/capi_layers.cpp), which makes the trainer's calls one for one:
  host  : Sampler::generateSubgraph + degree_counting + copy_to_gpu + compute_vertex_data + the row-by-row gather of the kept
          vertices' features and labels from host copies + their upload          (the path of the parent commit: the baseline)
  device: gaib_graph_induce + compute_vertex_data + gaib_gather_rows + gaib_gather_rows_u8 from the tables already in HBM
Both legs end in a stream wait inside the timed span (host wall clock).  One process, the legs ALTERNATING iteration by
iteration, 20 iterations per leg after 2 of warm-up, median and min-max per leg, the stream-copy rate of the run beside them.
Graphs: the products-shaped synthetic graph (graphaibench_amd.synth, with self loops, every vertex a training vertex, 100
features, 1 label byte) with vertex sets of about 10 K, 50 K and 200 K drawn by the host sampler, and the cora fixture
(tests/golden/cora, training range 0 .. 1500, 600 vertices asked for, 1433 features).  Before timing, both legs' subgraph,
feature rows and label rows are compared bit for bit.
For the device leg: the per-launch times of gaib_prof_table (a separate pass, in-stream events) and the algorithmic bytes of
the induce call -- the kept rows' edges x 4 B x 2 passes + the surviving edges x 4 B + the subgraph's row pointers x 8 B.
Reading rule: a leg is faster only if its median wins by more than both legs' spreads (max - min) together.

    python scripts/induce_subgraph.py OUT.json [--scale 1.0] [--iters 20] [--sizes 10000,50000,200000]
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from graphaibench_amd import capi, layers as L, synth  # noqa: E402

FRONTIER = 3000  # DEFAULT_SIZE_FRONTIER
INDUCE_KEYS = ("induce_mark", "induce_scan", "induce_count", "induce_fill")


def stats(ts):
    ts = sorted(ts)
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1], n=len(ts))


def verdict(ref, new):
    gain = ref["median_ms"] - new["median_ms"]
    spreads = (ref["max_ms"] - ref["min_ms"]) + (new["max_ms"] - new["min_ms"])
    return dict(gain_ms=gain, spreads_together_ms=spreads,
                reading="faster" if gain > spreads else ("slower" if -gain > spreads else "no difference beyond the spreads"))


def stream_copy_gbs(n_bytes=1 << 30, reps=10):
    x = torch.empty(n_bytes // 4, dtype=torch.float32, device="cuda").normal_()
    y = torch.empty_like(x)
    for _ in range(3):
        y.copy_(x)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        y.copy_(x)
    b.record()
    torch.cuda.synchronize()
    return 2.0 * n_bytes * reps / (a.elapsed_time(b) * 1e-3) / 1e9


def device_copy(ctx, ptr, n, dtype):
    out = torch.empty(n, dtype=dtype, device="cuda")
    if n:
        capi._check(ctx.lib.gaib_memcpy_d2d(ctx.h, out.data_ptr(), ptr, out.numel() * out.element_size()), "gaib_memcpy_d2d")
    ctx.sync()
    return out


def measure(ctx, name, rp, ci, masks, dim, sizes, iters, frontier=FRONTIER):
    """rp / ci: host CSR (numpy int64 / uint32); returns one record per vertex-set size"""
    lib = L.load()
    nv = len(rp) - 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_feats = torch.randn(nv, dim, device="cuda", generator=gen)
    d_labels = torch.randint(0, 7, (nv,), dtype=torch.uint8, device="cuda", generator=gen)
    feats, labels = d_feats.cpu().numpy(), d_labels.cpu().numpy()
    rp32 = np.ascontiguousarray(rp, np.uint32)
    ci32 = np.ascontiguousarray(ci, np.uint32)
    mk = np.ascontiguousarray(masks, np.uint8)
    h = lib.gaibl_sampling_create(nv, len(ci32), rp32.ctypes.data, ci32.ctypes.data, mk.ctypes.data, dim, 1, feats.ctypes.data,
                                  labels.ctypes.data, d_feats.data_ptr(), d_labels.data_ptr(), max(sizes))
    deg = np.diff(rp)
    records = []
    try:
        for want in sizes:
            n = int(lib.gaibl_sampling_select(h, want, min(frontier, want), 0))
            kept = np.empty(n, np.uint32)
            lib.gaibl_sampling_kept(h, kept.ctypes.data)
            # same results first: the subgraph, its feature rows and its label rows, bit for bit
            state = []
            for on_device in (0, 1):
                lib.gaibl_sampling_build(h, on_device)
                g = capi.Graph(ctx, _handle=C.c_void_p(lib.gaibl_sampling_ptr(h, 0)))
                g.close = lambda: None  # (owned by the hook)
                state.append((g.rowptr(), g.colidx(), g.vertex_data(),
                              device_copy(ctx, lib.gaibl_sampling_ptr(h, 1), n * dim, torch.float32),
                              device_copy(ctx, lib.gaibl_sampling_ptr(h, 2), n, torch.uint8)))
            same = all(torch.equal(a, b) for a, b in zip(*state))
            assert same, f"{name}: the device-built subgraph differs from the host-built one at {want} vertices"
            sub_ne = int(state[0][1].numel())
            del state
            for _ in range(2):
                for on_device in (0, 1):
                    lib.gaibl_sampling_build(h, on_device)
            t = {0: [], 1: []}
            for _ in range(iters):
                for on_device in (0, 1):
                    t[on_device].append(lib.gaibl_sampling_build(h, on_device))
            host, dev = stats(t[0]), stats(t[1])
            # the device leg's launches, in a pass of their own (events in the stream slow the host side down)
            ctx.prof_reset()
            ctx.prof_enable(True)
            prof_iters = 5
            for _ in range(prof_iters):
                lib.gaibl_sampling_build(h, 1)
            ctx.prof_enable(False)
            table = ctx.prof_table()
            ctx.prof_reset()
            kernels = {k: dict(count=v["count"], ms_per_call=v["ms"] / prof_iters) for k, v in table.items()}
            kept_edges = int(deg[kept].sum())
            alg_bytes = kept_edges * 4 * 2 + sub_ne * 4 + (n + 1) * 8
            induce_ms = sum(kernels[k]["ms_per_call"] for k in INDUCE_KEYS if k in kernels)
            records.append(dict(graph=name, nv=nv, ne=int(len(ci)), asked=want, kept=n, kept_rows_edges=kept_edges,
                                subgraph_edges=sub_ne, feature_columns=dim, same_results=bool(same), host=host, device=dev,
                                device_against_host=verdict(host, dev), device_kernels=kernels,
                                induce_algorithmic_bytes=alg_bytes, induce_kernels_ms=induce_ms,
                                induce_gbs=(alg_bytes / (induce_ms * 1e-3) / 1e9) if induce_ms > 0 else None))
            print(f"{name}: {n} kept: host {host['median_ms']:.3f} ms [{host['min_ms']:.3f}, {host['max_ms']:.3f}]  device "
                  f"{dev['median_ms']:.3f} ms [{dev['min_ms']:.3f}, {dev['max_ms']:.3f}]  induce kernels {induce_ms:.3f} ms",
                  flush=True)
    finally:
        lib.gaibl_sampling_free(h)
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the products-shaped graph (development only)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="10000,50000,200000")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    ctx = L.init(0)
    copy_before = stream_copy_gbs()
    records = []
    # cora: the fixture's topology with self loops, as the trainer samples it
    gold = ROOT / "tests" / "golden" / "cora"
    g0 = capi.Graph(ctx, np.fromfile(gold / "graph.vertex.bin", np.int64), np.fromfile(gold / "graph.edge.bin", np.uint32))
    g1 = g0.add_selfloop()
    rp, ci = g1.rowptr().cpu().numpy(), g1.colidx().cpu().numpy().view(np.uint32)
    g0.close(), g1.close()
    masks = np.zeros(len(rp) - 1, np.uint8)
    masks[:1500] = 1
    records += measure(ctx, "cora", rp, ci, masks, 1433, [600], args.iters)
    # the products-shaped graph
    sg = synth.make("ogbn-products", scale=args.scale)
    g0 = capi.Graph(ctx, sg.rowptr, sg.colidx)
    g1 = g0.add_selfloop()
    g0.close()
    del sg
    rp, ci = g1.rowptr().cpu().numpy(), g1.colidx().cpu().numpy().view(np.uint32)
    g1.close()
    torch.cuda.empty_cache()
    sizes = [max(16, int(int(s) * args.scale)) for s in args.sizes.split(",")]
    records += measure(ctx, "products-shaped (synth)", rp, ci, np.ones(len(rp) - 1, np.uint8), 100, sizes, args.iters)
    copy_after = stream_copy_gbs()
    out = dict(what="subgraph_sampling() after vertex selection: host path (parent commit) against option sampler_device",
               device=torch.cuda.get_device_name(0), iters_per_leg=args.iters, scale=args.scale,
               stream_copy_gbs=dict(before=copy_before, after=copy_after), cases=records)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(dict(stream_copy_gbs=out["stream_copy_gbs"], cases=len(records))))


if __name__ == "__main__":
    main()
