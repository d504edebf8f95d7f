"""gaib_sgemm_split (fp32 operands, both split exactly into three bf16 planes, nine plane products per term on the bf16 matrix
cores) against gaib_sgemm_ex with the option sgemm_split off, and the GCN and SAGE 256 -> 256 layer steps with the option off and
on.  One process; the legs of a comparison alternate call by call: 3 warm-up and 20 timed rounds per leg, device events around
each call; median (min - max) per leg, the stream-copy rate before and after.  A leg is called faster only if its median beats
the other's by more than the two min - max spreads together.  The kernels' register counts come from the notes of
the library's gfx950 code objects.  Fails without a GPU.

    python scripts/sgemm_split.py OUT.json [ROWS]

--tn: the weight gradients instead -- gaib_sgemm_split_tn (C = A^T . G over ROWS table rows, plain and with gaib_sgemm_drelu's
mask) against the fp32 route of the same call (gaib_sgemm_ex with transA = 1 / gaib_sgemm_drelu, option sgemm_split_tn off), and
the SAGE 256 -> 256 and GCN 128 -> 128 layer steps under sgemm_split alone and with sgemm_split_tn as well.

    python scripts/sgemm_split.py OUT.json [ROWS] --tn
"""
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from graphaibench_amd import capi, layers as L, synth  # noqa: E402

TN = "--tn" in sys.argv
ARGV = [a for a in sys.argv if a != "--tn"]
ROWS = int(ARGV[2]) if len(ARGV) > 2 else 2_449_029
ITERS, WARM = 20, 3
PAIRS = [(128, 128), (256, 256), (100, 128), (128, 256)]  # (K, N)
TN_PAIRS = [(128, 128), (256, 256), (100, 256)]  # (M, N) of the weight gradient
LLVM = Path("/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def alternate(legs):
    """legs: {name: callable}; -> {name: dict(median_ms, min_ms, max_ms, n)}, the legs taking turns"""
    for _ in range(WARM):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    evs = {k: [] for k in legs}
    for _ in range(ITERS):
        for k, f in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, v in evs.items():
        ts = sorted(a.elapsed_time(b) for a, b in v)
        out[k] = dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1], n=len(ts))
    return out


def verdict(new, old):
    spread = (new["max_ms"] - new["min_ms"]) + (old["max_ms"] - old["min_ms"])
    if old["median_ms"] - new["median_ms"] > spread:
        return "faster"
    if new["median_ms"] - old["median_ms"] > spread:
        return "slower"
    return "within the spread"


def kernel_registers(which="sgemm_split_kernel"):
    """{kernel: dict(vgpr, agpr, vgpr_spill, sgpr_spill)} of the sgemm_split kernels: every offload bundle of libgaib_hip.so's
    .hip_fatbin section, its gfx950 code object, the notes; "not measured" where the llvm tools are absent"""
    tools = [LLVM / "llvm-objcopy", LLVM / "clang-offload-bundler", LLVM / "llvm-readelf"]
    if not all(t.exists() for t in tools):
        return "not measured"
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = Path(tmp) / "fat.bin"
        subprocess.run([str(tools[0]), "-O", "binary", "--only-section=.hip_fatbin", str(capi.LIB_PATH), str(fat)], check=True)
        blob = fat.read_bytes()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for n, at in enumerate(starts):
            piece, co = Path(tmp) / f"b{n}.fat", Path(tmp) / f"b{n}.co"
            piece.write_bytes(blob[at:starts[n + 1] if n + 1 < len(starts) else len(blob)])
            r = subprocess.run([str(tools[1]), "--type=o", f"--input={piece}", "--unbundle",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not co.exists() or co.stat().st_size == 0:
                continue
            notes = subprocess.run([str(tools[2]), "--notes", str(co)], capture_output=True, text=True).stdout
            for k in re.findall(r"- \.agpr_count:.*?\.wavefront_size:", notes, re.S):
                name = re.search(r"\.name:\s+(\S+)", k)
                if name and which in name.group(1):
                    num = {f: int(re.search(rf"\.{f}:\s+(\d+)", k).group(1)) for f in ("agpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
                    found[name.group(1)] = dict(vgpr=num["vgpr_count"] - num["agpr_count"], agpr=num["agpr_count"], total=num["vgpr_count"],
                                                vgpr_spill=num["vgpr_spill_count"], sgpr_spill=num["sgpr_spill_count"])
    return found or "not measured"


def main_tn():
    ctx = L.init(0)
    rec = dict(rows=ROWS, iters=ITERS, kernels=kernel_registers("sgemm_split_tn_kernel"), stream_copy_gbs_before=ctx.probe_stream_copy(),
               products=[], layers=[])
    gen = torch.Generator(device="cuda").manual_seed(1)
    for M, N in TN_PAIRS:
        A = torch.randn(ROWS, M, device="cuda", generator=gen)
        G = torch.randn(ROWS, N, device="cuda", generator=gen) * 0.05
        mask = torch.sign(torch.randn(ROWS, N, device="cuda", generator=gen))
        Cf, Cs = torch.zeros(M, N, device="cuda"), torch.zeros(M, N, device="cuda")
        for masked in (False, True):  # (the masked call leaves G masked: every later call of either leg reads the same G)
            if masked:
                r = alternate(dict(fp32=lambda: ctx.sgemm_drelu(A, G, mask, Cf), split=lambda: ctx.sgemm_split_tn(A, G, Cs, mask=mask)))
            else:
                r = alternate(dict(fp32=lambda: ctx.sgemm(A, G, Cf, transA=True), split=lambda: ctx.sgemm_split_tn(A, G, Cs)))
            by = 4.0 * ROWS * (M + N * (3 if masked else 1)) + 4.0 * M * N
            row = dict(M=M, N=N, K=ROWS, form="masked" if masked else "plain", parts=ctx.sgemm_split_tn_parts(M, N, ROWS), **r,
                       split_alg_gbs=by / r["split"]["median_ms"] / 1e6, split_useful_tflops=2.0 * ROWS * N * M / r["split"]["median_ms"] / 1e9,
                       max_diff_rel=float((Cf - Cs).abs().max() / Cf.abs().max()), split_vs_fp32=verdict(r["split"], r["fp32"]))
            print(json.dumps(row), flush=True)
            rec["products"].append(row)
        del A, G, mask
        torch.cuda.empty_cache()
    sg = synth.make("ogbn-products", device="cuda", scale=ROWS / 2_449_029)
    g = ctx.graph(sg.rowptr, sg.colidx)
    ctx.sync()
    nv = g.nv
    lg = L.LGraph.adopt(g)
    opt = L.adam(0.01)
    for kind, d, name in ((L.SAGE, 256, "sage_256_256"), (L.GCN, 128, "gcn_128_128")):
        layer = L.Layer(kind, 1, nv, d, d, lg, True)
        layer.write(L.FEAT_IN, torch.randn(nv, d, device="cuda"))
        layer.write(L.GRAD_IN, torch.randn(nv, d, device="cuda"))
        out, gout = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")

        def step(on):
            ctx.set_option("sgemm_split_tn", on)
            layer.forward(out)
            layer.backward(out, gout)
            layer.update_weight(opt)

        ctx.set_option("sgemm_split", 1)
        try:
            r = alternate(dict(split=lambda: step(0), split_wgrad=lambda: step(1)))
        finally:
            ctx.set_option("sgemm_split", 0)
            ctx.set_option("sgemm_split_tn", 0)
        rec["layers"].append(dict(layer=name, nv=nv, **r, split_wgrad_vs_split=verdict(r["split_wgrad"], r["split"])))
        print(json.dumps(rec["layers"][-1]), flush=True)
        layer.close()
        del out, gout
        torch.cuda.empty_cache()
    rec["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    L.adam_free(opt)
    Path(ARGV[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(ARGV[1]).write_text(json.dumps(rec, indent=1) + "\n")


def main():
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    if TN:
        return main_tn()
    ctx = L.init(0)
    rec = dict(rows=ROWS, iters=ITERS, kernels=kernel_registers(), stream_copy_gbs_before=ctx.probe_stream_copy(), products=[], layers=[])
    gen = torch.Generator(device="cuda").manual_seed(1)
    for K, N in PAIRS:
        x = torch.randn(ROWS, K, device="cuda", generator=gen)
        Cf, Cs = torch.zeros(ROWS, N, device="cuda"), torch.zeros(ROWS, N, device="cuda")
        for transB in (False, True):
            B = torch.randn((N, K) if transB else (K, N), device="cuda", generator=gen) * 0.05
            r = alternate(dict(fp32=lambda: ctx.sgemm(x, B, Cf, transB=transB), split=lambda: ctx.sgemm_split(x, B, Cs, transB=transB)))
            by = 4.0 * ROWS * K + 4.0 * ROWS * N + 4.0 * K * N
            worst = float((Cf - Cs).abs().max() / Cf.abs().max())  # (two summation orders of the same exact terms)
            row = dict(M=ROWS, N=N, K=K, form="NT" if transB else "NN", **r, split_alg_gbs=by / r["split"]["median_ms"] / 1e6,
                       split_useful_tflops=2.0 * ROWS * N * K / r["split"]["median_ms"] / 1e9, max_diff_rel=worst,
                       split_vs_fp32=verdict(r["split"], r["fp32"]))
            print(json.dumps(row), flush=True)
            rec["products"].append(row)
        del x, Cf, Cs
        torch.cuda.empty_cache()
    # the GCN and SAGE 256 -> 256 layer steps on the products-shaped graph, fp32 tables
    sg = synth.make("ogbn-products", device="cuda", scale=ROWS / 2_449_029)
    g = ctx.graph(sg.rowptr, sg.colidx)
    ctx.sync()
    nv, d = g.nv, 256
    lg = L.LGraph.adopt(g)
    opt = L.adam(0.01)
    for kind, name in ((L.GCN, "gcn_256_256"), (L.SAGE, "sage_256_256")):
        layer = L.Layer(kind, 1, nv, d, d, lg, True)
        layer.write(L.FEAT_IN, torch.randn(nv, d, device="cuda"))
        layer.write(L.GRAD_IN, torch.randn(nv, d, device="cuda"))
        out, gout = torch.empty(nv, d, device="cuda"), torch.empty(nv, d, device="cuda")

        def step(on):
            ctx.set_option("sgemm_split", on)
            layer.forward(out)
            layer.backward(out, gout)
            layer.update_weight(opt)

        try:
            r = alternate(dict(fp32=lambda: step(0), split=lambda: step(1)))
        finally:
            ctx.set_option("sgemm_split", 0)
        rec["layers"].append(dict(layer=name, nv=nv, **r, split_vs_fp32=verdict(r["split"], r["fp32"])))
        print(json.dumps(rec["layers"][-1]), flush=True)
        layer.close()
        del out, gout
        torch.cuda.empty_cache()
    rec["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    L.adam_free(opt)
    Path(ARGV[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(ARGV[1]).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
