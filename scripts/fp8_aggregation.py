"""fp8 feature tables with per-row scales on the products-shaped bench graph (synth, N = 2 449 029, E = 125.9 M with self
loops), next to fp32 and bf16 tables.

    python scripts/fp8_aggregation.py OUT.json [--scale 1.0] [--iters 20] [--no-quality] [--no-timing]

Every timed group is INTERLEAVED: one call of every leg per round, --iters rounds (at least 20) after warm-up, so that box and
clock state are shared; median, min and max per leg, the stream-copy rate before and after.  Each width is first checked bit for
bit against the fp32 call on the widened table.
  plain   gaib_spmm (fp32) | gaib_spmm_bf16_ld at gaib_bf16_row_stride's stride | gaib_spmm_fp8, GCN weights, at 47, 100, 128 and
          256 columns; algorithmic bytes count 4 / 2 / 1 B per gathered element (+ 4 B of scale per edge for fp8)
  fused   gaib_spmm_gemm | _bf16 | _fp8 at 128 -> 128, aggregate kept
  cast    gaib_cast_f32_bf16_rows | gaib_cast_f32_fp8_rows alone, at the same widths
  layers  GCN 128 -> 128 and SAGE 128 -> 128 layer steps (forward + backward + update) under agg_bf16 / agg_fp8 / neither
  quality through the trainer binaries (bin/gpu_train_gcn, GAIB_AGG_DTYPE = fp32 | bf16 | fp8, GAIB_EPOCH_LOSSES = 1): cora's
          topology and labels with synthetic learnable features -- the dataset of the bf16 trainer test -- as a 2-layer GCN with
          hidden width 16, and in that test's configuration (hidden width 64); the loss curve and the final train accuracy of
          each table format over the same feature seeds
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from graphaibench_amd import capi, layers as L, synth  # noqa: E402

GOLD = ROOT / "tests" / "golden"


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


def apart(a, b):
    """two legs differ when their medians are apart by more than both min-max spreads together"""
    return bool(abs(a["median_ms"] - b["median_ms"]) > (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"]))


def timing(args, rec):
    iters = max(args.iters, 20)
    ctx = L.init(0)
    sg = synth.make("ogbn-products", device="cuda", scale=args.scale)
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g = g0.add_selfloop()
    g0.close()
    ctx.sync()
    nv, ne = g.nv, g.ne
    rec.update(graph="ogbn-products synth", nv=nv, ne=ne, iters=iters, stream_copy_gbs_before=ctx.probe_stream_copy(), plain=[], cast=[],
               fused=[], layers=[])
    print(f"nv={nv} ne={ne} stream copy {rec['stream_copy_gbs_before']:.0f} GB/s", flush=True)
    none = lambda: None
    bits = lambda t: t.view(torch.int32)

    def opts(**kw):
        def setup():
            for k, v in kw.items():
                ctx.set_option(k, v)
        return setup

    for d in (47, 100, 128, 256):
        x = torch.randn(nv, d, device="cuda")
        ld16 = ctx.bf16_row_stride(g, d)
        xb = ctx.cast_f32_bf16_rows(x, ld16)
        q, scale = ctx.cast_f32_fp8_rows(x)
        out, ref = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")
        xw = ctx.cast_fp8_f32_rows(q, scale, d)
        ctx.spmm(g, capi.W_GCN, xw, ref)
        ctx.spmm_fp8(g, capi.W_GCN, q, scale, out)
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(ref)), f"fp8 aggregation differs from fp32 on the widened table at {d}"
        del xw
        torch.cuda.empty_cache()
        legs = dict(fp32=(none, lambda: ctx.spmm(g, capi.W_GCN, x, ref)),
                    bf16=(none, lambda: ctx.spmm_bf16(g, capi.W_GCN, xb, out, ld=ld16)),
                    fp8=(none, lambda: ctx.spmm_fp8(g, capi.W_GCN, q, scale, out)))
        r = dict(d=d, kind="W_GCN", ld_bf16=ld16, ld_fp8=q.shape[1], bit_identical=True, legs=interleaved(legs, iters))
        for k, eb in (("fp32", 4.0), ("bf16", 2.0), ("fp8", 1.0)):  # gathered row + col id + weight (+ scale), output, row pointers
            nbytes = ne * (eb * d + 8 + (4 if k == "fp8" else 0)) + nv * 4.0 * d + (nv + 1) * 8.0
            r["legs"][k]["frac_8tbs"] = nbytes / r["legs"][k]["median_ms"] / 1e6 / 8000
        r["fp8_apart_from_bf16"] = apart(r["legs"]["fp8"], r["legs"]["bf16"])
        r["fp8_apart_from_fp32"] = apart(r["legs"]["fp8"], r["legs"]["fp32"])
        print(json.dumps(r), flush=True)
        rec["plain"].append(r)
        c = dict(d=d, legs=interleaved(dict(bf16=(none, lambda: ctx.cast_f32_bf16_rows(x, ld16, xb)),
                                            fp8=(none, lambda: ctx.cast_f32_fp8_rows(x, q.shape[1], q, scale))), iters))
        print(json.dumps(c), flush=True)
        rec["cast"].append(c)
        if d == 128:
            W = torch.randn(d, d, device="cuda") * 0.1
            agg, agg_r = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")
            xw = ctx.cast_fp8_f32_rows(q, scale, d)
            ctx.spmm_gemm(g, capi.W_GCN, xw, agg_r, W, ref)
            ctx.spmm_gemm_fp8(g, capi.W_GCN, q, scale, agg, W, out)
            torch.cuda.synchronize()
            assert torch.equal(bits(out), bits(ref)) and torch.equal(bits(agg), bits(agg_r)), "fused fp8 call differs from the fp32 call on the widened table"
            del xw, agg_r
            torch.cuda.empty_cache()
            legs = dict(fp32=(none, lambda: ctx.spmm_gemm(g, capi.W_GCN, x, agg, W, out)),
                        bf16=(none, lambda: ctx.spmm_gemm_bf16(g, capi.W_GCN, xb, agg, W, out, ld=ld16)),
                        fp8=(none, lambda: ctx.spmm_gemm_fp8(g, capi.W_GCN, q, scale, agg, W, out)))
            f = dict(shape="128->128", kind="W_GCN", bit_identical=True, legs=interleaved(legs, iters))
            f["fp8_apart_from_bf16"] = apart(f["legs"]["fp8"], f["legs"]["bf16"])
            print(json.dumps(f), flush=True)
            rec["fused"].append(f)
            del W, agg
        del x, xb, q, scale, out, ref
        torch.cuda.empty_cache()

    lg = L.LGraph.adopt(g)
    try:
        for kind, name in ((L.GCN, "gcn_128_128"), (L.SAGE, "sage_128_128")):
            layer = L.Layer(kind, 1, nv, 128, 128, lg, True)
            layer.write(L.FEAT_IN, torch.randn(nv, 128, device="cuda"))
            out, gout = torch.empty(nv, 128, device="cuda"), torch.empty(nv, 128, device="cuda")
            opt = L.adam(0.01)
            layer.write(L.GRAD_IN, torch.randn(nv, 128, device="cuda"))

            def step():
                layer.forward(out)
                layer.backward(out, gout)
                layer.update_weight(opt)

            legs = dict(fp32=(opts(agg_fp8=0, agg_bf16=0), step), bf16=(opts(agg_fp8=0, agg_bf16=1), step),
                        fp8=(opts(agg_bf16=0, agg_fp8=1), step))
            r = dict(layer=name, legs=interleaved(legs, iters))
            r["fp8_apart_from_bf16"] = apart(r["legs"]["fp8"], r["legs"]["bf16"])
            r["fp8_apart_from_fp32"] = apart(r["legs"]["fp8"], r["legs"]["fp32"])
            print(json.dumps(r), flush=True)
            rec["layers"].append(r)
            L.adam_free(opt)
            layer.close()
            del out, gout
            torch.cuda.empty_cache()
    finally:
        ctx.set_option("agg_bf16", 0)
        ctx.set_option("agg_fp8", 0)
    rec["stream_copy_gbs_after"] = ctx.probe_stream_copy()


def make_dataset(root, feat_len, seed):
    """root/cora/: cora's topology and labels with synthetic learnable features (tests/test_gpu_bf16.py: make_dataset)"""
    d = Path(root) / "cora"
    d.mkdir(parents=True)
    for f in ("graph.vertex.bin", "graph.edge.bin", "graph.vlabel.bin"):
        shutil.copyfile(GOLD / "cora" / f, d / f)
    meta = (GOLD / "cora" / "graph.meta.txt").read_text().split()
    meta[7] = str(feat_len)
    (d / "graph.meta.txt").write_text("\n".join(meta) + "\n")
    rng = np.random.default_rng(seed)
    labels = np.fromfile(d / "graph.vlabel.bin", np.uint8)
    x = rng.standard_normal((2708, feat_len)).astype(np.float32) * 0.5
    x[np.arange(2708), labels.astype(int) % feat_len] += 1.5
    x.tofile(d / "graph.feats.bin")


def quality(args, rec):
    rec["quality"] = []
    exe = ROOT / "bin" / "gpu_train_gcn"
    for name, hidden, epochs in (("cora_gcn_hidden16", "16", "50"), ("cora_gcn_hidden64", "64", "20")):
        for seed in (0, 1, 2):
            with tempfile.TemporaryDirectory() as tmp:
                make_dataset(tmp, 96, seed)
                runs = {}
                for dt in ("fp32", "bf16", "fp8"):
                    env = dict(os.environ, DATASET_PATH=tmp + "/", GAIB_AGG_DTYPE=dt, GAIB_EPOCH_GRAPH="0", GAIB_EPOCH_LOSSES="1")
                    cmd = [str(exe), "cora", epochs, "2", "softmax", hidden, "0", "0", "0.01", "2", "0", "4", "0"]
                    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
                    if r.returncode != 0:
                        raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
                    text = r.stdout + r.stderr
                    losses = [float(v) for v in re.search(r"epoch_losses ([0-9eE.+\- naif]+)", text).group(1).split()]
                    m = re.search(r"epoch_accs ([0-9eE.+\- naif]+)", text)
                    accs = [float(v) for v in m.group(1).split()] if m else [float(a) for a in re.findall(r"train_acc ([0-9.]+)", text)]
                    runs[dt] = dict(losses=losses, final_train_acc=accs[-1] if accs else None)
                q = dict(model=name, feature_seed=seed, epochs=int(epochs), runs=runs)
                print(json.dumps(dict(model=name, seed=seed, **{dt: (v["losses"][0], v["losses"][-1], v["final_train_acc"]) for dt, v in runs.items()})),
                      flush=True)
                rec["quality"].append(q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    args = ap.parse_args()
    rec = {}
    if not args.no_quality:  # (first: the trainer processes run while this one has not opened the GPU)
        quality(args, rec)
    if not args.no_timing:
        timing(args, rec)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
