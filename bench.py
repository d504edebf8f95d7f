#!/usr/bin/env python3
"""bench.py -- GCN-layer forward+backward on an ogbn-products-shaped graph, 1..8 MI355X.

Metric (BASELINE.json): "GCN-layer fwd+bwd: aggregated edges/sec + achieved HBM GB/s".
A step = one pass of the hot path: GCN_layer(128 -> 128, hidden layer, relu)::forward +
::backward on the host C++ layer API (include/layers/graph_conv_layer.h) over the C ABI
(include/gaib.h): 2 SpMM at D=128 + 3 fp32 MFMA GEMMs + relu + d_relu.
`value` = aggregated edges (2 * E per step, E incl. self loops, summed over ranks) / wall time,
inputs resident in HBM when the timed region starts.

    python bench.py --gpus N --steps K --warmup W
    N > 1, either way:
      * plainly, as above: with no WORLD_SIZE in the environment bench.py is its own launcher -- the parent touches no
        GPU API, starts N fresh rank processes (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*), relays rank 0's JSON line
        as its last stdout line, and on the first failing rank or at --deadline-s kills the rest and exits non-zero
        (one entry point drives all devices, like the reference's multi-GPU programs: src/triangle/multigpu_induced.cu:31-84);
      * python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...  (the ranks given from outside).
    Ranks map to devices as LOCAL_RANK % visible devices; with fewer devices than ranks (a one-GPU box) the data path is
    the peer-to-peer pull transport, which lets several ranks share a device, and the record says so (config.transport,
    config.ranks_share_device, roofline.ranks_share_device: such timings are evidence of nothing).

    What an N > 1 run measures (round 5; DESIGN.md 5 "which figure is value"):
      `value`  north_star's curve -- the N = 1 bench graph (products shape, seed 42, random vertex order) partitioned N ways by
               vertex range (graph_partition.cc:128-178), "scaling": "strong"; config.strong_products repeats it with the
               one-rank timing of the same graph taken in the run (speedup_vs_n1).  Its parity is element-wise against the
               oracle's run on the WHOLE graph (the run the N = 1 bench makes), whose timing is also the record's cpu_baseline.
      second   config.weak_products_range: a products-shaped vertex range per GPU of one block graph at cut 0.1 (--scaling weak
               swaps the two), then config.cu_reserve_ab and config.transport_ab -- the run measures its own constants on the
               live headline case -- config.xgmi_link_probe (measured FIRST and fed to the partition-mode rule before any
               partition exists), the weak generator's parity legs at bounded size, config.clustered_boundary,
               config.random_order, and at N = 8 config.config5_papers100M.
    The N > 1 record cannot be lost: the headline case runs first and rank 0 HOLDS its record (RecordGuard: SIGTERM / SIGINT
    blocked as main()'s first act, before torch is imported, so no native thread can take them); every further leg starts
    only if all ranks agree that it fits --budget-s (420 s; else its slot says {"skipped": "budget", ...}); on --deadline-s
    (560 s), a signal, or an exception on any rank after the headline case rank 0 prints what it holds, marked "partial",
    with parity = {"ok": null, "reason"} if the comparison had not completed, and exits 0.  A heartbeat line goes to stderr
    every minute.  The N = 1, GAT and epoch records are held the same way once their GPU measurement is complete.
    --workload gcn-papers: BASELINE config 5's layer (GCN 128 -> 128 on the ogbn-papers100M-shaped graph in vertex ranges
    of 1/8 of it: at N = 8 the whole graph); --check-oracle compares every rank's outputs with the oracle's GLOBAL run.
    --workload gat-reddit: config 4's layer; with --gpus N (round 6) on a vertex-range partition of the reddit-shaped graph -- the
    one-rank step of the same layer is taken in the run and rank 0's rows are held to it (dist.bench_gat_layer).
    --workload epoch-sage-products | epoch-gcn-products | epoch-gat-reddit | epoch-gcn-cora [--hidden H]: one training EPOCH of the
    model configs through the trainer CLI per step (bench_epoch).  The N = 1 run with --full appends configs 2-4 as budgeted legs
    (`other_configs`, --other-configs-s) after the headline record is held.

One JSON line on rank 0.  `roofline` prices the dominant kernel (spmm_gemm_kernel: the one-wave-per-row
aggregation with the dense product riding on it) by ALGORITHMIC bytes per launch / mean launch time measured
with HIP events in the timed region.  A plain N = 1 run stops there: set-up, warm-up, the timed steps, the record.
With --full it adds the stream-copy rate measured in the same run (roofline.peak_measured); `cpu_baseline` times
the oracle's restatement of the OpenMP path on the host on the SAME graph and inputs, and `parity` compares the
GPU layer's forward output, input gradient and weight gradient with that run element by element (exit code 3
above 1e-4); `sustained_ms_per_step` is the same step kept up for >= 5 s after the timed region; then the
planted-locality leg and the other_configs block.  --dump-outputs DIR writes what the last timed step computed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

D = 128  # feature width of the layer under test (north star: D = 128)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured stream copy)


T_START = time.time()  # the process's start: what --budget-s and --deadline-s count from


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def start_heartbeat(who: str, every_s: float = 60.0) -> None:
    """a line on stderr every minute: a harness that watches a run's output takes minutes of silence for a hang and kills the
    run (the pool's limit is 7 minutes -- shorter than --deadline-s), and the oracle's legs on the host are silent for that long
    at full size on few cores"""
    def beat():
        while True:
            time.sleep(every_s)
            log(f"[bench {who}] alive, {time.time() - T_START:.0f} s since start")

    threading.Thread(target=beat, daemon=True, name="bench-heartbeat").start()


def usable_cores() -> int:
    """CPUs this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, q // per))
        except Exception:
            pass
    return max(1, n)


def blob_hash(path: Path) -> str:
    """`git hash-object` of a file (the GPU box has the tree, not the repository)"""
    import hashlib

    data = path.read_bytes()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def traffic_from_profile(key: str, section: str | None = None):
    """per-launch L2 -> fabric bytes of a kernel from the committed PMC summary (profiles/hbm_traffic.json: separate
    rocprofv3 --pmc passes of this very command -- counters cannot be read inside the timed run).  The summary names the
    kernel sources it was taken with (`sources`: path -> git blob hash); if any of them differs from the tree that is
    running, the figure belongs to other kernels and is DROPPED (None + the reason) instead of being reported.
    Returns (traffic_bytes_per_launch | None, source_or_reason)."""
    tf = ROOT / "profiles" / "hbm_traffic.json"
    if not tf.exists():
        return None, "profiles/hbm_traffic.json missing"
    try:
        tj = json.loads(tf.read_text())
        sec = tj.get(section, {}) if section else tj
        srcs = sec.get("sources") or {}
        if not srcs:
            return None, "dropped: profiles/hbm_traffic.json names no kernel sources to check against"
        for rel, want in srcs.items():
            path = ROOT / rel
            if not path.exists() or blob_hash(path) != want:
                return None, (f"dropped: {rel} changed since the PMC passes at commit {sec.get('commit', '?')} "
                              f"(re-run scripts/profile_round.sh + scripts/make_hbm_traffic.py)")
        val = sec.get(key)
        if not val:
            return None, f"dropped: {key} not in profiles/hbm_traffic.json"
        return float(val), (f"profiles/hbm_traffic.json{' ' + section if section else ''} (rocprofv3 --pmc passes at commit "
                            f"{sec.get('commit', '?')}; kernel sources verified by blob hash)")
    except Exception as e:  # a malformed summary must not take the bench line down
        return None, f"dropped: {type(e).__name__}: {e}"


def host_inputs(nv: int):
    """the layer's inputs, generated ONCE on the host (seed 43) and fed to BOTH legs: the GPU layer and
    the CPU oracle see the same X and the same incoming gradient, so their outputs are comparable element-wise."""
    import numpy as np

    rng = np.random.default_rng(43)
    x = rng.standard_normal((nv, D), dtype=np.float32)
    gin = rng.standard_normal((nv, D), dtype=np.float32)
    return x, gin


DUMP_ROWS = 32768  # rows of each N x D output written by --dump-outputs: 2 x 16 MiB at D = 128


def dump_outputs(out_dir: Path, torch, L, layer, feat_out, grad_out) -> None:
    """--dump-outputs: what the caller of the timed step receives, as float32 .npy -- the layer output and the input gradient
    at a fixed sample of rows (seed 0, ascending), and the whole weight gradient"""
    import numpy as np

    nv, din, dout = layer.nv, layer.din, layer.dout
    rows = np.arange(nv) if nv <= DUMP_ROWS else np.sort(np.random.default_rng(0).choice(nv, DUMP_ROWS, replace=False))
    rows_d = torch.from_numpy(rows).cuda()
    out_dir.mkdir(parents=True, exist_ok=True)
    arrays = {"feat_out": feat_out[rows_d], "grad_out": grad_out[rows_d], "w_grad": layer.tensor(L.W_NEIGH_GRAD, (din, dout))}
    for name, t in arrays.items():
        np.save(out_dir / f"{name}.npy", t.float().cpu().numpy())
    log(f"[bench] outputs of the last timed step written to {out_dir}: {', '.join(arrays)} ({len(rows)} of {nv} rows)")


def cpu_baseline(sg_rowptr, sg_colidx, nv, x, gin, budget_s=30.0, want_outputs=True):
    """The oracle (port of the reference's OpenMP GCN layer, oracle/gnn_oracle.c) on the host cores, on the SAME
    graph and the SAME inputs as the GPU leg.  Returns (cpu_baseline record, outputs of the full-graph run or None).
    The full graph is run whenever parity is wanted; its time is the baseline when it fits the budget, otherwise a
    bounded row-prefix sample [0, R) is timed."""
    import ctypes as C

    import numpy as np
    from oracle import binding as orc

    cores = usable_cores()
    orc.set_threads(cores)
    rp = sg_rowptr.cpu().numpy()
    ci = sg_colidx.cpu().numpy().view(np.uint32)
    g_full = orc.Graph(rp, ci).add_selfloop()  # net.cpp:96
    vd = g_full.vertex_data()
    W = orc.init_glorot(D, D, 1)
    libs = {"lib": orc.lib()}
    p = orc._p
    # scratch of the layer (graph_conv_layer.cpp:10-36), allocated once outside the timed region like the ctor does
    in_temp = np.zeros((nv, D), np.float32)
    in_temp1 = np.zeros((nv, D), np.float32)
    out_temp = np.zeros((nv, D), np.float32)

    def run(R, keep=False):
        g = orc.Graph.__new__(orc.Graph)
        g.rowptr, g.colidx, g.nv, g.ne, g.vd = g_full.rowptr[:R + 1], g_full.colidx, R, int(g_full.rowptr[R]), vd
        s = g._struct()
        out = np.empty((R, D), np.float32)
        grad_out = np.zeros((R, D), np.float32)
        W_grad = np.zeros((D, D), np.float32)
        g_in = gin[:R].copy()  # backward applies d_relu to it in place (Q9)
        lib = libs["lib"]
        t0 = time.perf_counter()
        # feature tables keep ALL rows: the aggregation gathers any column
        lib.orc_gcn_layer_forward(C.byref(s), C.c_int(D), C.c_int(D), C.c_int(1), p(x), p(W), p(in_temp1[:R]),
                                  p(out_temp[:R]), p(out))
        lib.orc_gcn_layer_backward(C.byref(s), C.c_int(1), C.c_int(D), C.c_int(D), C.c_int(1), p(x), p(W), p(out),
                                   p(g_in), p(in_temp), p(in_temp1[:R]), p(out_temp[:R]), p(grad_out), p(W_grad))
        t = time.perf_counter() - t0
        return t, 2 * g.ne, (dict(forward=out, grad_out=grad_out, W_grad=W_grad, agg_x=in_temp1[:R].copy(),
                                  masked_grad=g_in) if keep else None)

    probe_R = max(nv // 64, 1024)
    run(min(probe_R, nv))  # thread spin-up: the first pass is ~2x slower
    t_probe, e_probe, _ = run(min(probe_R, nv))
    rate = e_probe / max(t_probe, 1e-9)
    total_edges = 2 * g_full.ne
    fits = total_edges / rate <= budget_s
    outputs = None
    if want_outputs or fits:
        t, e, outputs = run(nv, keep=want_outputs)
        R = nv
    if not fits:
        R = min(max(int(nv * budget_s * rate / total_edges), probe_R), nv)
        t, e, _ = run(R)
    res = dict(value=e / t, unit="edges/s", cores=cores, cores_available=os.cpu_count(),
               cores_note=f"threads = the {cores} cores this process may use (affinity mask / cgroup quota) of the host's "
                          f"{os.cpu_count()}; SURVEY 8d's 32-thread figure needs a host share of >= 32 cores",
               kind="port",
               sample=f"rows [0,{R}) of the same graph ({e // 2} edges incl. self loops), 1 layer fwd+bwd on the GPU "
                      f"leg's inputs, {t:.2f} s, gcc -O3 -fopenmp no -march=native (reference Makefile flags)")
    # how the reference would run it (src/gnn/Makefile:50-54 links MKL or OpenBLAS; env.sh:3-6 sets OMP_NUM_THREADS=32 and
    # KMP_AFFINITY=scatter): `value` keeps the port's own blocked sgemm -- the run the parity leg compares with is that one --
    # and the same sample is timed once more with the three dense products through cblas_sgemm of libmkl_rt where it loads
    res["gemm"] = "builtin (the port's blocked sgemm; value_mkl_sgemm: the same sample with the layer's products through cblas_sgemm)"
    res["omp"] = {"threads": cores, "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS"), "OMP_PROC_BIND": os.environ.get("OMP_PROC_BIND"),
                  "OMP_PLACES": os.environ.get("OMP_PLACES"),
                  "note": "reference env.sh: OMP_NUM_THREADS=32, KMP_AFFINITY=scatter (Intel runtime); libgomp's equivalent is "
                          "OMP_PROC_BIND=spread, set by bench.py before the runtime starts unless the caller set it"}
    try:
        if orc.use_blas(True):
            run(min(probe_R, nv))  # (MKL's first call builds its thread pool)
            tb, eb, _ = run(R)
            res["value_mkl_sgemm"] = eb / tb
        else:
            res["value_mkl_sgemm"] = None
            res["gemm"] += "; no cblas library could be loaded on this host"
    except Exception as ex:  # noqa: BLE001 -- a second figure must not cost the first
        res["value_mkl_sgemm"] = {"error": f"{type(ex).__name__}: {ex}"[:200]}
    finally:
        orc.use_blas(False)
    nat = orc.native_lib()  # another figure with -march=native built on this host, same sample
    if nat is not None:
        libs["lib"] = nat
        run(min(probe_R, nv))
        tn, en, _ = run(R)
        res["value_march_native"] = en / tn
    return res, outputs


def _errs(torch, a, b, tol, floor):
    """(elem, inf) of device tensor a against device tensor b, fp64, chunked"""
    a, b = a.reshape(-1), b.reshape(-1)
    scale = max(b.abs().max().item(), 1e-30)
    elem = inf = 0.0
    step = 1 << 26
    for i in range(0, a.numel(), step):
        bb = b[i:i + step].double()
        d = (a[i:i + step].double() - bb).abs()
        inf = max(inf, d.max().item() / scale)
        elem = max(elem, (d / (bb.abs() + (floor / tol) * scale)).max().item())
    return {"elem": elem, "inf": inf}


def flips_against_fp64(torch, layer, L, graph, feat_in, feat_out, fwd_o, flips, D_):
    """The outputs whose relu mask differs between the GPU and the oracle, evaluated in fp64 from the layer's inputs: a flipped
    mask bit is two CORRECT roundings of the same number only if that number is within the fp32 rounding of its own sum of
    zero -- |y64| <= bound, bound = (terms of the sum) * 2^-24 * sum|terms| of the row (aggregation) and of the dot product.
    Anchors the "backward on the oracle's mask" criterion in the exact value instead of in the two implementations.
    graph: the layer's device graph (A + I, rows sorted); weights as the aggregation forms them: vd[i] * vd[c] in fp32."""
    idx = torch.nonzero(flips)
    if idx.numel() == 0:
        return {"count": 0}
    idx = idx[:256]  # (a handful in practice)
    rp, ci, vd = graph.rowptr(), graph.colidx().to(torch.int64), graph.vertex_data()
    W = layer.tensor(L.W_NEIGH, (D_, D_)).double()
    worst = worst_ratio = 0.0
    for i, j in idx.tolist():
        e0, e1 = int(rp[i]), int(rp[i + 1])
        cols = ci[e0:e1]
        w = (vd[i] * vd[cols]).double()                      # (the fp32 product of the kernel, then exact)
        rows = feat_in[cols].double()
        a = (w[:, None] * rows).sum(0)                        # aggregated row, fp64
        a_abs = (w[:, None].abs() * rows.abs()).sum(0)
        y = float((a * W[:, j]).sum())
        y_abs = float((a_abs * W[:, j].abs()).sum())
        bound = ((e1 - e0) + D_) * 2.0 ** -24 * y_abs         # first-order bound of an fp32 evaluation in any order
        worst = max(worst, abs(y))
        worst_ratio = max(worst_ratio, abs(y) / max(bound, 1e-300))
    scale = float(fwd_o.abs().max())
    return {"count": int(flips.sum().item()), "checked": int(idx.shape[0]), "max_abs_fp64_value_over_scale": worst / scale,
            "max_abs_fp64_value_over_fp32_rounding_bound": worst_ratio,
            "ok": bool(worst_ratio <= 1.0),
            "note": "every output whose mask bit differs is, evaluated in fp64 from the inputs, within the first-order fp32 rounding "
                    "bound of its own sum around zero: both signs are correct fp32 roundings"}


def parity_record(torch, L, layer, feat_out, grad_out, gin_h, want: dict, tol=1e-4, floor=1e-6, graph=None, feat_in=None):
    """Element-wise parity of the GPU layer against the oracle's full-graph run on the same inputs.

    Per tensor: `elem` = max_i |a_i-b_i| / (|b_i| + (floor/tol) max|b|)  (<= tol  <=>  |a-b| <= tol|b| + floor max|b|
    for every element) and `inf` = max|a-b| / max|b|, on the device in fp64.

    forward is compared as is.  backward depends on the relu mask (d_relu masks with the layer's OUTPUT > 0, Q9): an
    output within rounding of zero can land on either side in two correct fp32 evaluations, and one flipped mask bit
    moves a whole gradient row by O(1).  So backward is compared twice: `*_own_mask` with the mask the GPU's own forward
    produced (the raw end-to-end figure; a handful of flips among 3e8 elements dominate it) and `grad_out` / `W_grad`
    with the GPU backward re-run on the ORACLE's forward output as feat_out (identical masks: arithmetic error only).
    `relu_mask_flips` counts the differing mask bits and gives the largest |output| among them -- they must all sit
    within rounding of zero for the run to pass."""
    D_ = want["W_grad"].shape[0]
    nv = want["forward"].shape[0]
    rec = {"tol": tol, "floor_frac_of_max": floor}
    fwd_o = torch.from_numpy(want["forward"]).cuda()
    rec["forward"] = _errs(torch, feat_out, fwd_o, tol, floor)
    flips = (feat_out > 0) != (fwd_o > 0)
    n_flips = int(flips.sum().item())
    scale = fwd_o.abs().max().item()
    worst = max(feat_out[flips].abs().max().item(), fwd_o[flips].abs().max().item()) / scale if n_flips else 0.0
    rec["relu_mask_flips"] = {"count": n_flips, "of": int(fwd_o.numel()), "max_abs_output_over_scale": worst}
    if graph is not None and feat_in is not None:
        try:
            rec["relu_mask_flips"]["fp64"] = flips_against_fp64(torch, layer, L, graph, feat_in, feat_out, fwd_o, flips, D_)
        except Exception as e:  # noqa: BLE001 -- an extra check must not cost the record
            rec["relu_mask_flips"]["fp64"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    del flips
    go_o = torch.from_numpy(want["grad_out"]).cuda()
    wg_o = torch.from_numpy(want["W_grad"]).cuda()
    rec["grad_out_own_mask"] = _errs(torch, grad_out, go_o, tol, floor)
    rec["W_grad_own_mask"] = _errs(torch, layer.tensor(L.W_NEIGH_GRAD, (D_, D_)), wg_o, tol, floor)
    # the same backward kernels on the oracle's mask
    layer.write(L.GRAD_IN, torch.from_numpy(gin_h).cuda())
    layer.backward(fwd_o, grad_out)
    torch.cuda.synchronize()
    rec["grad_out"] = _errs(torch, grad_out, go_o, tol, floor)
    w_gpu = layer.tensor(L.W_NEIGH_GRAD, (D_, D_))
    rec["W_grad"] = _errs(torch, w_gpu, wg_o, tol, floor)
    del go_o, fwd_o
    # the weight gradient is a sum over 2.4 M vertices in fp32 on both sides; where the truth lies: fp64 on the device
    ax = torch.from_numpy(want["agg_x"]).cuda().double()
    mg = torch.from_numpy(want["masked_grad"]).cuda().double()
    w64 = ax.t() @ mg
    sc = w64.abs().max().item()
    gpu64 = (w_gpu.double() - w64).abs().max().item() / sc
    orc64 = (wg_o.double() - w64).abs().max().item() / sc
    rec["W_grad_vs_fp64_inf"] = {"gpu": gpu64, "oracle": orc64}
    # W_grad is a sum over the 2.4 M vertices, in fp32 on both sides: the oracle's own result sits `orc64` * max|b| away
    # from fp64, so no evaluation can match it element-wise below that.  Its floor is therefore twice the ORACLE's own
    # distance from fp64 (never the GPU's: a wrong GPU result must not widen its own tolerance), at least the default.
    w_floor = max(floor, 2.0 * orc64)
    rec["W_grad"]["elem_floor"] = w_floor
    rec["W_grad"]["elem_at_floor"] = _errs(torch, w_gpu, wg_o, tol, w_floor)["elem"]
    rec["ok"] = bool(rec["forward"]["elem"] <= tol and rec["forward"]["inf"] <= tol
                     and rec["grad_out"]["elem"] <= tol and rec["grad_out"]["inf"] <= tol
                     and rec["W_grad"]["inf"] <= tol and rec["W_grad"]["elem_at_floor"] <= tol
                     and gpu64 <= 2e-5 and worst <= 1e-5
                     and rec["relu_mask_flips"].get("fp64", {}).get("ok", True) is not False)
    return rec


class DistOracleCheck:
    """--check-oracle on the partitioned path: every rank's share of the layer's forward output and input gradient, and
    the weight gradient summed over the ranks, against the oracle's run on the GLOBAL graph (the block generator is
    seeded per range, so rank 0 regenerates every range and joins them; rows keep the global column order).  Same
    scheme as parity_record: forward as is, backward re-run on the ORACLE's forward output (identical relu masks).
    The partitioned aggregation adds a row's owned-column edges before its halo-column edges -- another order than
    the oracle's ascending columns -- so every row is a re-ordered fp32 sum: floor 1e-5 max|b| (tests/util.py
    LONG_SUM_FLOOR), the weight gradient's floor from the oracle's own distance to fp64 as in parity_record."""

    TOL, FLOOR = 1e-4, 1e-5
    exchanger = None  # set by dist._bench_case: the layer's own halo exchanger (diagnostics)

    def __init__(self, torch, dist, synth, L, gdist, ctx, comm, args, rank, world, shape, cut, boundary="uniform", bounds=None,
                 graph_fn=None):
        self.torch, self.dist, self.synth, self.L, self.gdist = torch, dist, synth, L, gdist
        self.ctx, self.comm, self.args, self.rank, self.world, self.shape, self.cut = ctx, comm, args, rank, world, shape, cut
        self.boundary = boundary  # the generator of the case under test (synth.block_rows)
        # the strong case: ONE given global graph (graph_fn() -> the oracle's graph, self loops in; rank 0 only) cut at `bounds`
        # (gdist.partition_bounds: the last range may be shorter); its oracle run is also the N = 1 workload's CPU baseline
        self.bounds, self.graph_fn = bounds, graph_fn

    @staticmethod
    def inputs(rank: int, nv: int):
        import numpy as np

        rng = np.random.default_rng(4300 + rank)
        return rng.standard_normal((nv, D), dtype=np.float32), rng.standard_normal((nv, D), dtype=np.float32)

    def _sizes(self, nv):
        """rows per rank: the cut of the given graph, or `world` equal ranges of the block generator"""
        if self.bounds is not None:
            return [self.bounds[q + 1] - self.bounds[q] for q in range(self.world)]
        return [nv] * self.world

    def _oracle_global(self, nv):
        import numpy as np
        from oracle import binding as orc

        torch, synth = self.torch, self.synth
        sizes = self._sizes(nv)
        cores = usable_cores()
        orc.set_threads(cores)
        if self.graph_fn is not None:
            g = self.graph_fn()
            assert g.nv == sum(sizes), (g.nv, sizes)
        else:
            rps, cis, off = [np.zeros(1, np.int64)], [], 0
            for q in range(self.world):
                rows = synth.block_rows(self.shape, q, self.world, seed=42, cut_fraction=self.cut, device="cuda",
                                        scale=self.args.scale, selfloops=True, boundary=self.boundary, band=0.2)
                assert rows.n_local == nv
                rps.append(rows.rowptr[1:].cpu().numpy() + off)
                cis.append(rows.colidx_global.cpu().numpy().astype(np.uint32))
                off += int(rows.rowptr[-1])
                del rows
            torch.cuda.empty_cache()
            g = orc.Graph(np.concatenate(rps), np.concatenate(cis))  # self loops are in (block_rows(selfloops=True), net.cpp:96)
        xs = [self.inputs(q, sizes[q]) for q in range(self.world)]
        x, gin = np.concatenate([a for a, _ in xs]), np.concatenate([b for _, b in xs])
        del xs
        if self.graph_fn is not None:  # its time is reported as a CPU baseline: thread spin-up out of the way first
            R = max(min(g.nv // 64, 50000), 1)
            gs = orc.Graph.__new__(orc.Graph)
            gs.rowptr, gs.colidx, gs.nv, gs.ne, gs.vd = g.rowptr[:R + 1], g.colidx, R, int(g.rowptr[R]), g.vertex_data()
            s_, p_ = gs._struct(), orc._p
            import ctypes as C

            t1, t2, o_ = np.zeros((R, D), np.float32), np.zeros((R, D), np.float32), np.empty((R, D), np.float32)
            orc.lib().orc_gcn_layer_forward(C.byref(s_), C.c_int(D), C.c_int(D), C.c_int(1), p_(x), p_(orc.init_glorot(D, D, 1)),
                                            p_(t1), p_(t2), p_(o_))
        lay = orc.GCNLayer(1, g, D, D, True)
        t0 = time.perf_counter()
        fwd = lay.forward(x)
        go = lay.backward(gin)  # gin is masked in place (Q9)
        t = time.perf_counter() - t0
        return dict(forward=fwd, grad_out=go, W_grad=lay.W_grad, agg_x=lay.in_temp1, masked_grad=gin, seconds=t,
                    edges=g.ne, nv=g.nv, cores=cores)

    def __call__(self, part, layer, feat_out, grad_out):
        torch, dist, L = self.torch, self.dist, self.L
        nv = part.n_own
        x_h, gin_h = self.inputs(self.rank, nv)
        want, err = None, [None]
        if self.rank == 0:  # (a failing oracle run -- host memory, say -- must not leave the other ranks in a collective)
            try:
                want = self._oracle_global(nv)
            except Exception as e:  # noqa: BLE001
                err[0] = f"{type(e).__name__}: {e}"[:300]
        dist.broadcast_object_list(err, src=0)
        if err[0]:
            return {"error": err[0], "ok": None} if self.rank == 0 else None
        # rank 0 hands every rank its rows of the oracle's outputs (control plane: gloo / the launcher's group)
        sizes = self._sizes(nv)
        offs = [sum(sizes[:q]) for q in range(self.world + 1)]
        nmax = max(sizes)

        def scatter(key):  # (scatter wants equal shapes: a shorter last range is padded)
            mine = torch.empty(nmax, D)
            parts = None
            if self.rank == 0:
                parts = []
                for q in range(self.world):
                    t_ = torch.from_numpy(want[key][offs[q]:offs[q + 1]])
                    if sizes[q] < nmax:
                        t_ = torch.cat([t_, torch.zeros(nmax - sizes[q], D)])
                    parts.append(t_.contiguous())
            if dist.get_backend() == "nccl":
                mine = mine.cuda()
                parts = [p_.cuda() for p_ in parts] if parts else None
            dist.scatter(mine, parts, src=0)
            return mine[:nv].cuda().contiguous()

        fwd_o, go_o = scatter("forward"), scatter("grad_out")
        layer.write(L.FEAT_IN, torch.from_numpy(x_h).cuda())
        layer.forward(feat_out)
        torch.cuda.synchronize()
        e_f = _errs(torch, feat_out, fwd_o, self.TOL, self.FLOOR)
        flips = int(((feat_out > 0) != (fwd_o > 0)).sum().item())
        if os.environ.get("GAIB_BENCH_PARITY_DEBUG") and (e_f["elem"] > self.TOL or e_f["inf"] > self.TOL):
            d = (feat_out - fwd_o).abs().amax(1) / fwd_o.abs().max().clamp_min(1e-30)
            bad = torch.nonzero(d > 1e-4).flatten()
            log(f"[bench r{self.rank}] PARITY DEBUG forward: {bad.numel()} of {nv} rows off by > 1e-4 of max; first {bad[:12].tolist()} "
                f"last {bad[-6:].tolist()}; worst row {int(d.argmax())} ({float(d.max()):.3e}); rows with halo edges among the bad: "
                f"{int((part.rowptr_halo[1:] - part.rowptr_halo[:-1])[bad].gt(0).sum())}")
        if os.environ.get("GAIB_BENCH_PARITY_DEBUG") and self.exchanger is not None:
            # the halo table itself: one exchange of x through the layer's plan against the rows the peers hold (collective)
            import numpy as np

            x_all = np.concatenate([self.inputs(q, nv)[0] for q in range(self.world)])
            got = self.exchanger.exchange(torch.from_numpy(x_h).cuda(), D)
            want_t = torch.from_numpy(x_all[part.halo_gids.cpu().numpy()]).cuda()
            badr = torch.nonzero((got != want_t).any(1)).flatten()
            offs = np.cumsum([0] + list(part.recv_counts))
            log(f"[bench r{self.rank}] PARITY DEBUG halo table: {badr.numel()} of {part.n_halo} rows differ; first {badr[:16].tolist()} "
                f"last {badr[-8:].tolist()}; segment offsets {offs.tolist()}; send offsets {np.cumsum([0] + list(part.send_counts)).tolist()}")
            del x_all, got, want_t
        layer.write(L.GRAD_IN, torch.from_numpy(gin_h).cuda())
        layer.backward(fwd_o, grad_out)  # the oracle's forward output: identical relu masks
        self.gdist.allreduce_layer_grads(self.ctx, layer, [L.W_NEIGH_GRAD], (D, D), comm=self.comm)
        torch.cuda.synchronize()
        e_g = _errs(torch, grad_out, go_o, self.TOL, self.FLOOR)
        t = torch.tensor([e_f["elem"], e_f["inf"], e_g["elem"], e_g["inf"], float(flips)], dtype=torch.float64)
        if dist.get_backend() == "nccl":
            t = t.cuda()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        rec = None
        if self.rank == 0:
            w_gpu = layer.tensor(L.W_NEIGH_GRAD, (D, D))
            wg_o = torch.from_numpy(want["W_grad"]).cuda()
            w64 = torch.from_numpy(want["agg_x"]).cuda().double().t() @ torch.from_numpy(want["masked_grad"]).cuda().double()
            sc = w64.abs().max().item()
            gpu64 = (w_gpu.double() - w64).abs().max().item() / sc
            orc64 = (wg_o.double() - w64).abs().max().item() / sc
            w_floor = max(self.FLOOR, 2.0 * orc64)
            e_w = _errs(torch, w_gpu, wg_o, self.TOL, w_floor)
            rec = {"tol": self.TOL, "floor_frac_of_max": self.FLOOR, "against": "oracle GCN layer on the GLOBAL graph "
                   f"({want['nv']} vertices, {want['edges']} edges incl. self loops, {want['seconds']:.1f} s on the host), "
                   f"max over {self.world} ranks", "cut_fraction": self.cut,
                   "forward": {"elem": float(t[0]), "inf": float(t[1])}, "grad_out": {"elem": float(t[2]), "inf": float(t[3])},
                   "relu_mask_flips_max_per_rank": int(t[4]),
                   "W_grad": {**e_w, "elem_floor": w_floor}, "W_grad_vs_fp64_inf": {"gpu": gpu64, "oracle": orc64}}
            rec["ok"] = bool(max(float(v) for v in t[:4]) <= self.TOL and e_w["elem"] <= self.TOL and e_w["inf"] <= self.TOL
                             and gpu64 <= 2e-5)
            if self.graph_fn is not None:
                # the oracle's run on the N = 1 bench graph, whole, on the run's inputs: the N = 1 workload's CPU baseline
                # (gdist.bench_gcn_layer moves it to the record's cpu_baseline)
                rec["cpu_baseline"] = dict(
                    value=2 * want["edges"] / want["seconds"], unit="edges/s", cores=want["cores"], cores_available=os.cpu_count(),
                    kind="port",
                    sample=f"the whole N = 1 bench graph ({want['nv']} vertices, {want['edges']} edges incl. self loops), 1 GCN layer "
                           f"fwd+bwd, {want['seconds']:.2f} s on rank 0's host cores while the other ranks wait, gcc -O3 -fopenmp no "
                           f"-march=native (reference Makefile flags); the same run the strong case's parity is checked against",
                    of="the N = 1 workload (ogbn-products shape, seed 42): the graph this run partitions")
            log(f"[bench] parity vs the oracle's GLOBAL run (cut {self.cut:.3f}): {rec}")
        dist.barrier()
        return rec


_REAL_STDOUT = None  # the process's original fd 1, once quiet_stdout() has pointed fd 1 at stderr


def quiet_stdout() -> None:
    """stdout carries ONE line, the record.  Libraries underneath print to fd 1 on their own (gloo: "[Gloo] Rank 0 is
    connected to 1 peer ranks", RCCL: its library path), from every rank: from here on fd 1 IS stderr, and emit() writes the
    JSON line to the saved original."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def emit(result: dict) -> None:
    """the ONE JSON line, last on stdout (C stdio buffers of the libraries flushed first, wherever they point)"""
    import ctypes
    sys.stdout.flush()
    ctypes.CDLL(None).fflush(None)
    os.write(_REAL_STDOUT if _REAL_STDOUT is not None else 1, (json.dumps(result) + "\n").encode())


def profiler_preload() -> str:
    """non-empty if this process runs under a profiler that preloads a GPU-touching library (rocprofv3 / rocprofiler-sdk)"""
    if os.environ.get("ROCP_TOOL_LIBRARIES"):
        return "ROCP_TOOL_LIBRARIES is set"
    for var in ("LD_PRELOAD", "HSA_TOOLS_LIB"):
        v = os.environ.get(var, "")
        if "rocprof" in v or "roctracer" in v or "rocprofiler" in v:
            return f"{var} names a profiler library ({v[:80]})"
    return ""


def launch_ranks(args, argv, entry=None) -> int:
    """`python bench.py --gpus N` without ranks from outside: start them.  This parent imports no torch and calls no
    GPU API (a process that has touched the GPU must never be replaced or forked into ranks on this pool); every rank
    is a FRESH interpreter in a session of its own.  Rank 0's stdout is collected (its last JSON line is relayed as
    this process's last stdout line), everything else of every rank goes to stderr.  Supervision: the first rank that
    exits non-zero, or the wall-clock deadline, ends the run -- the remaining ranks (exactly the process groups started
    here) get SIGTERM, then SIGKILL, and the exit status is non-zero.  That is also the watchdog the RCCL transport
    lacks on its own (a rank waiting in a collective for a dead peer has no deadline inside RCCL).
    entry: the rank program (default: this file; the CPU tests of the supervision pass a stand-in)."""
    import signal
    import socket
    import subprocess

    why = profiler_preload()
    if why:  # the tool library has initialised the GPU in THIS process already: starting ranks from it is the forbidden exec
        log(f"[bench launcher] {why}: a profiler's preloaded library touches the GPU before main, and a process that has "
            "must not start rank programs on this pool.  Profile ONE rank program directly after `--` (ranks from outside: "
            "RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT set per process), or profile the N = 1 run.")
        return 2
    n = args.gpus
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:  # a free rendezvous port on the loopback
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    nonce = f"{os.getpid()}-{int(time.time())}"
    procs, lines = [], []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GAIB_LAUNCH_NONCE=nonce)
        procs.append(subprocess.Popen([sys.executable, str(entry or Path(__file__).resolve()), *argv], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr, text=True,
                                      start_new_session=True))

    def pump():
        for line in procs[0].stdout:
            lines.append(line.rstrip("\n"))

    th = threading.Thread(target=pump, daemon=True)
    th.start()

    def stop_all(sig):
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, sig)  # the session (= process group) started above, nothing else
                except ProcessLookupError:
                    pass

    def on_signal(signum, frame):
        # the driver (or a user) ends the run from outside: the ranks get SIGTERM, rank 0 prints the record it holds (RecordGuard,
        # which may wait up to 5 s for a record that is about to be held), and THAT line is relayed before this process leaves
        log(f"[bench launcher] signal {signum}: stopping the ranks")
        stop_all(signal.SIGTERM)
        t_end = time.time() + 9
        while time.time() < t_end and any(p.poll() is None for p in procs):
            time.sleep(0.1)
        stop_all(signal.SIGKILL)
        th.join(timeout=3)
        out = [l for l in lines if l.startswith("{")]
        if out and procs[0].poll() == 0:
            print(out[-1], flush=True)
        os._exit(128 + signum)

    signal.signal(signal.SIGTERM, on_signal)
    signal.signal(signal.SIGINT, on_signal)
    deadline = time.time() + args.deadline_s
    rc, why = 0, ""
    rank0_done_at, stragglers = None, False
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            rc, why = (bad[0][1] if bad[0][1] > 0 else 128 - bad[0][1]), f"rank {bad[0][0]} exited with {bad[0][1]}"
            break
        if all(c == 0 for c in codes):
            break
        # rank 0 has left with status 0 -- its record is out (in full, or the one it held when something failed on it) -- and
        # the others are still there, e.g. inside a collective rank 0 will never join: they get 20 s, not the whole deadline
        if codes[0] == 0:
            rank0_done_at = rank0_done_at or time.time()
            if time.time() - rank0_done_at > 20.0:
                stragglers = True
                log(f"[bench launcher] rank 0 exited 0 more than 20 s ago, stopping ranks {[r for r, c in enumerate(codes) if c is None]}")
                break
        if time.time() > deadline:
            rc, why = 124, f"deadline of {args.deadline_s:.0f} s passed (ranks still running: " \
                           f"{[r for r, c in enumerate(codes) if c is None]})"
            break
        time.sleep(0.1)
    if rc or stragglers:
        if rc:
            log(f"[bench launcher] {why}: stopping the other ranks")
        stop_all(signal.SIGTERM)
        t_end = time.time() + 10
        while time.time() < t_end and any(p.poll() is None for p in procs):
            time.sleep(0.1)
        stop_all(signal.SIGKILL)
    th.join(timeout=10)
    out = [l for l in lines if l.startswith("{")]
    for l in lines:
        if not out or l is not out[-1]:
            log(l)
    if rc == 0 and not out:
        log("[bench launcher] rank 0 printed no JSON line")
        rc = 1
    # a record rank 0 DID emit is relayed whatever ended the run (exit 3 / 4: its own verdict on the record; 5: a leg after the
    # headline case crashed, the held record is out; exit 0 after
    # the deadline or a signal: the record it held, marked partial -- RecordGuard)
    if out and (rc == 0 or procs[0].poll() in (0, 3, 4, 5)):
        print(out[-1], flush=True)
        if rc == 124 and procs[0].poll() == 0:  # the deadline cut the sub-cases short, the headline record is out
            rc = 0
    return rc


# ---- child programs (the trainer CLI of the epoch workloads) ---------------------------------------------------------------
# main() blocks SIGTERM / SIGINT first thing and a signal mask survives fork + exec: a child started plainly would run with both
# blocked, and RecordGuard.bail() -- deadline or signal -- leaves through os._exit without a look at it: an orphan on the GPU
# that ignores SIGTERM, under the next GPU step.  So: every child starts in a session of its own through a
# two-line wrapper that restores the mask BEFORE it becomes the program (an exec in a fresh interpreter that has touched no GPU),
# its handle is kept here, and bail() kills and reaps the whole group before it leaves.
_CHILDREN = []
_CHILDREN_LOCK = threading.Lock()
_UNMASK = ("import os, signal, sys; signal.pthread_sigmask(signal.SIG_UNBLOCK, {signal.SIGTERM, signal.SIGINT}); "
           "os.execv(sys.argv[1], sys.argv[1:])")


def kill_children(grace_s: float = 0.0) -> int:
    """SIGTERM (if grace_s > 0), then SIGKILL, to the process group of every child still alive, and reap them -> how many"""
    import signal
    import subprocess

    with _CHILDREN_LOCK:
        alive = [p for p in _CHILDREN if p.poll() is None]
    for sig, wait_s in ((signal.SIGTERM, grace_s), (signal.SIGKILL, 5.0)):
        if sig == signal.SIGTERM and grace_s <= 0:
            continue
        for p in alive:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, sig)
                except (ProcessLookupError, PermissionError):
                    pass
        t_end = time.time() + wait_s
        for p in alive:
            try:
                p.wait(timeout=max(0.0, t_end - time.time()))
            except subprocess.TimeoutExpired:
                pass
    return len(alive)


def run_child(cmd, env=None, timeout_s: float = 600.0, unmask=_UNMASK):
    """cmd as a supervised child (see above) -> (returncode, stdout, stderr).  On timeout the group is killed and
    subprocess.TimeoutExpired raised."""
    import subprocess

    p = subprocess.Popen([sys.executable, "-c", unmask, *[str(c) for c in cmd]], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, start_new_session=True)
    with _CHILDREN_LOCK:
        _CHILDREN.append(p)
    try:
        out, err = p.communicate(timeout=timeout_s)
    except subprocess.TimeoutExpired:
        kill_children()
        raise
    finally:
        with _CHILDREN_LOCK:
            if p.poll() is not None and p in _CHILDREN:
                _CHILDREN.remove(p)
    return p.returncode, out, err


class RecordGuard:
    """The N > 1 record cannot be lost: rank 0 HOLDS the record as soon as the headline case is measured (hold), the
    sub-cases that follow only add to it, and whatever ends the run early -- the deadline, SIGTERM from the launcher or the
    driver, a sub-case that hangs in a collective -- makes rank 0 print the record it holds, marked `partial`, and exit 0.
    Exactly one JSON line leaves the process (final / bail race under a lock).  The watchers are THREADS (a timer, and
    sigwait on the blocked SIGTERM / SIGINT): a Python signal handler would not run while the main thread sits in a C call."""

    def __init__(self, rank: int):
        self.rank, self.lock, self.held, self.done = rank, threading.Lock(), None, False
        self.leaving = threading.Event()  # set once a bail() owns the exit: a second caller waits for it instead of racing it out
        self.want_parity = False  # the run was asked for a comparison with the oracle: a record cut short must SAY it has none

    def hold(self, record: dict) -> None:
        with self.lock:
            self.held = record

    def final(self, record: dict) -> None:
        with self.lock:
            if not self.done:
                self.done = True
                emit(record)

    def bail(self, reason: str, status: int = 0) -> None:
        """from a watcher thread (deadline, signal) or from an exception handler (a leg after the measurement crashed): print
        what is held (rank 0) and leave with `status`.  A held record that was to carry `parity` and does not gets
        parity = {"ok": null, "reason": ...}, next to `partial`: UNCHECKED, never silently the same as checked (the
        exit status stays 0 so that whoever collects the line keeps the measured headline -- the marker is what says the run
        did not end the way a passing run does)."""
        with self.lock:
            if self.done:
                # the record is out already (final), or another thread's bail() is on its way out -- it killed the child program
                # this thread was waiting for, which is why this thread is here: let IT print and leave, do not outrun it
                if self.leaving.is_set():
                    time.sleep(30)
                return
            self.done = True
            self.leaving.set()
            held = self.held
        n_killed = kill_children()  # (a trainer child of an epoch leg: never left behind on the GPU)
        if n_killed:
            log(f"[bench r{self.rank}] {reason}: killed {n_killed} child program(s)")
        if self.rank == 0 and held is None:
            # the headline case may just have ended: between its last collective and hold() rank 0 still assembles the record
            # (milliseconds) -- a peer that fails exactly then makes the launcher's SIGTERM arrive first.  Give the main thread
            # a moment to hand the record over before giving up (it never comes if the main thread sits in a collective).
            for _ in range(50):
                time.sleep(0.1)
                with self.lock:
                    held = self.held
                if held is not None:
                    break
        if self.rank == 0 and held is not None:
            held = dict(held)
            held["partial"] = {"reason": reason, "note": "the headline case was measured in full; sub-cases that had not "
                                                          "finished are null or say why"}
            if self.want_parity and not isinstance(held.get("parity"), dict):
                held["parity"] = {"ok": None, "reason": f"the comparison with the oracle did not complete: {reason}"}
            log(f"[bench r0] {reason}: printing the record held so far (exit {status})")
            emit(held)
            os._exit(status)
        log(f"[bench r{self.rank}] {reason}: exiting 124")
        os._exit(124)


def install_rank_guard(rank: int, deadline_s: float) -> RecordGuard:
    """inside a rank: a collective that waits for a dead peer never returns (RCCL has no deadline of its own), so the
    rank ends itself when the run's deadline passes -- under torch.distributed.run that ends the job as well -- and on
    SIGTERM / SIGINT; rank 0 prints the record it holds first (RecordGuard)"""
    import signal

    guard = RecordGuard(rank)
    sigs = {signal.SIGTERM, signal.SIGINT}
    # main() has blocked both already, as its FIRST act in a rank / N = 1 process -- before `import torch` and any HIP call, so
    # that every native thread created later (HSA's event thread, the OpenMP pool) inherits the mask; a thread that predates
    # the mask would take a process-directed SIGTERM at SIG_DFL and the record would die with it.  Again here for
    # callers that come without main() (the tests' stand-in rank programs).
    signal.pthread_sigmask(signal.SIG_BLOCK, sigs)

    def wait_signal():
        s = signal.sigwait(sigs)
        guard.bail(f"signal {s}")

    threading.Thread(target=wait_signal, daemon=True).start()
    t = threading.Timer(deadline_s, lambda: guard.bail(f"deadline of {deadline_s:.0f} s passed"))
    t.daemon = True
    t.start()
    return guard


def main():
    if os.environ.get("GAIB_BENCH_DUMP_STACKS_S"):  # diagnosis of a stuck rank: every process writes its Python stacks to stderr
        import faulthandler

        faulthandler.dump_traceback_later(float(os.environ["GAIB_BENCH_DUMP_STACKS_S"]), repeat=True, file=sys.stderr)
    if os.environ.get("GAIB_RCCL_LIB"):  # (tests/fake_rccl's double is for call-pattern tests; a record must name the real RCCL)
        sys.exit("bench.py: GAIB_RCCL_LIB is set -- the bench measures the system's RCCL only; unset it")
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (development only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the element-wise comparison with the oracle's run")
    ap.add_argument("--sustain-s", type=float, default=5.0,
                    help="after the timed steps, run the same step for this many seconds (0 = skip; N = 1 GCN record: with --full)")
    ap.add_argument("--cut-fraction", type=float, default=None,
                    help="N>1, weak scaling: fraction of each partition's edges that cross partitions (default: 0.1 as "
                         "`value` and (N-1)/N as config.random_order, both in one run)")
    ap.add_argument("--workload", choices=["gcn-products", "gat-reddit", "gcn-papers", *EPOCH_WORKLOADS], default="gcn-products",
                    help="gcn-products: BASELINE's headline (default).  gat-reddit: BASELINE config 4, one 8-head GAT layer "
                         "64 -> 64 forward + backward on the reddit-shaped graph (same JSON schema; one GPU).  gcn-papers: "
                         "BASELINE config 5's layer, GCN 128 -> 128 on the ogbn-papers100M-shaped graph, one vertex range of "
                         "1/8 of it per GPU (N = 8: the whole graph), halo rows + dW over the collectives.  epoch-*: BASELINE "
                         "configs 2-4 are MODELS -- one training epoch of the 3-layer GraphSAGE (hidden 256, "
                         "scripts/run-sage-products.sh) / 3-layer GCN (hidden 128) on the products shape, of the 2-layer 8-head GAT "
                         "on the reddit shape, through the trainer CLI (a step = one epoch; same JSON schema; one GPU)")
    ap.add_argument("--hidden", type=int, default=None,
                    help="epoch-* workloads: the hidden width (default the workload's own; epoch-sage-products: 256 as "
                         "scripts/run-sage-products.sh passes it, `--hidden 128` = BASELINE config 3's literal \"3-layer D=128\")")
    ap.add_argument("--other-configs-s", type=float, default=float(os.environ.get("GAIB_BENCH_OTHER_CONFIGS_S", "100")),
                    help="N = 1 run with --full: wall-clock budget of the `other_configs` block -- BASELINE configs 2-4 as short legs "
                         "after the headline record is held (SAGE layer steps at 128 / 256, the 8-head GAT layer, the epoch "
                         "workloads); 0 = skip")
    ap.add_argument("--no-locality", action="store_true",
                    help="skip the planted-locality leg of the N = 1 record (profiling runs: its launches of the dominant kernel "
                         "on ANOTHER graph would be averaged into the per-kernel statistics)")
    ap.add_argument("--check-oracle", action="store_true",
                    help="N>1 (or gcn-papers): compare every rank's forward output, input gradient and the summed weight "
                         "gradient element-wise with the oracle's run on the GLOBAL graph (sizes the host finishes in "
                         "seconds: use --scale); exit code 3 above 1e-4")
    ap.add_argument("--deadline-s", type=float, default=float(os.environ.get("GAIB_BENCH_DEADLINE_S", "560")),
                    help="wall-clock limit of the run, any N (under the 600 s the driver grants a bench run), counted from the "
                         "process's start: N>1 -- the launcher stops all ranks, a rank ends itself; N=1 (GCN and GAT lines) -- the "
                         "legs after the GPU measurement (CPU baseline, parity) are cut.  Rank 0 prints the record it holds first, "
                         "marked `partial`, with parity = {ok: null, reason} if the comparison had not completed; exit 0 (the same "
                         "when a leg after the measurement raises)")
    ap.add_argument("--budget-s", type=float, default=float(os.environ.get("GAIB_BENCH_BUDGET_S", "420")),
                    help="N>1: wall-clock budget of the whole run, counted from the rank's start.  The headline case always runs; "
                         "every further sub-case (CPU baseline, random vertex order, config 5) starts only if all ranks agree that "
                         "its estimated time still fits, else the record says {\"skipped\": \"budget\", ...}")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="strong",
                    help="N>1, which case is `value`: strong (default) = the single-GPU bench graph partitioned N ways (north_star's "
                         "\"edges/sec at 1/2/4/8\" on ogbn-products: total work fixed); weak = one products-shaped vertex range per "
                         "GPU at --cut-fraction.  A default run measures BOTH: the other one is config.weak_products_range / "
                         "config.strong_products.  gcn-papers (config 5) is weak by construction")
    ap.add_argument("--full", action="store_true",
                    help="N = 1 GCN record: also run the legs beside the headline -- the sustained leg, the in-run stream-copy "
                         "probe (roofline.peak_measured), the planted-locality leg, the CPU baseline with the element-wise "
                         "comparison against the oracle, and the other_configs block.  Without it the N = 1 run sets up, warms "
                         "up, times --steps steps and prints the record")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="N = 1 GCN record: after the timed steps write what the last timed step computed as float32 .npy files "
                         "under DIR -- feat_out / grad_out (the layer output and the input gradient at 32768 rows drawn with "
                         "seed 0, ascending; every row if the graph has fewer) and w_grad (the whole D x D weight gradient)")
    args = ap.parse_args()
    if args.dump_outputs and (args.gpus > 1 or args.workload != "gcn-products"):
        ap.error("--dump-outputs is written by the N = 1 gcn-products record")
    if args.workload in EPOCH_WORKLOADS and args.gpus > 1:
        ap.error(f"--workload {args.workload} is a one-GPU workload; N > 1 runs gcn-products, gcn-papers or gat-reddit")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        sys.exit(launch_ranks(args, sys.argv[1:]))  # no torch, no GPU API in this process

    # A rank / N = 1 process from here on.  FIRST: SIGTERM / SIGINT are blocked and the watcher threads started (sigwait + the
    # deadline timer), before torch is imported and before any HIP call -- every thread created after this line inherits the
    # mask, so a process-directed signal can only be taken by the sigwait thread, which prints the held record.
    import signal

    signal.pthread_sigmask(signal.SIG_BLOCK, {signal.SIGTERM, signal.SIGINT})
    os.environ.setdefault("OMP_PROC_BIND", "spread")  # (the CPU baseline's threads like the reference's KMP_AFFINITY=scatter; before any OpenMP runtime starts)
    quiet_stdout()
    guard = install_rank_guard(int(os.environ.get("RANK", "0")), max(5.0, args.deadline_s - (time.time() - T_START)))
    # (N = 1: the comparison needs the CPU baseline's run; N > 1: the strong case's comparison is its own leg)
    guard.want_parity = (not args.no_parity and (int(os.environ.get("WORLD_SIZE", "1")) > 1 or not args.no_cpu_baseline)) or args.check_oracle
    if int(os.environ.get("RANK", "0")) == 0:
        start_heartbeat("r0")
    import torch

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        log(f"[bench] --gpus {args.gpus} but WORLD_SIZE={world}: give bench.py the ranks (torch.distributed.run "
            f"--nproc-per-node {args.gpus}) or none at all (it starts them itself)")
        sys.exit(2)
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    ndev = torch.cuda.device_count()
    device = local_rank % ndev
    if world > 1:
        if world > ndev and "GAIB_DIST_BACKEND" not in os.environ:
            # ranks share devices (a one-GPU box): RCCL refuses that by design, the peer-to-peer pull transport does not
            os.environ["GAIB_DIST_BACKEND"] = "ipc"
            log(f"[bench r{rank}] {world} ranks on {ndev} device(s): data path = gaib_comm/ipc (several ranks per device)")
    torch.cuda.set_device(device)

    from graphaibench_amd import capi, layers as L, synth

    ctx = L.init(device)
    for kv in filter(None, os.environ.get("GAIB_OPTS", "").split(",")):  # development knobs: GAIB_OPTS="key=value,..."
        k, v = kv.split("=")
        ctx.set_option(k.strip(), int(v))
        log(f"[bench] option {k.strip()} = {int(v)}")

    # the env knob runs the N>1 code on one GPU; config 5's workload is defined on the partitioned path at any N
    if world > 1 or os.environ.get("GAIB_FORCE_DIST") == "1" or args.workload == "gcn-papers":
        import torch.distributed as dist
        from graphaibench_amd import dist as gdist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        # data path: gaib_comm behind the C ABI (GAIB_DIST_BACKEND = rccl (default) | ipc), or torch.distributed itself
        # (nccl | gloo).  torch.distributed is the control plane either way (the communicator id, barriers, the max-over-
        # ranks timing): gloo over 127.0.0.1 unless the data path is torch's nccl
        backend = os.environ.get("GAIB_DIST_BACKEND", "rccl")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        make_check = None
        if args.check_oracle:
            make_check = lambda shape, cut, comm: DistOracleCheck(torch, dist, synth, L, gdist, ctx, comm, args, rank, world,
                                                                  shape, cut)
        launcher = ("bench.py itself (parent without GPU state, fresh rank processes, supervised)"
                    if os.environ.get("GAIB_LAUNCH_NONCE") else "ranks given from outside (torch.distributed.run)")

        def hold(record):  # (rank 0) the headline case is measured: from here on the record cannot be lost
            if rank == 0:
                record["config"]["launcher"] = launcher
                guard.hold(record)

        def cpu_leg(budget_s):  # (rank 0) the N = 1 workload's CPU baseline on a bounded sample, named as such
            sg = synth.make("ogbn-products", seed=42, device="cuda", scale=min(args.scale, 0.1))
            x_h, gin_h = host_inputs(sg.nv)
            rec, _ = cpu_baseline(sg.rowptr, sg.colidx, sg.nv, x_h, gin_h, budget_s=budget_s, want_outputs=False)
            rec["of"] = (f"the N = 1 workload (ogbn-products shape, seed 42) at scale {min(args.scale, 0.1)}: {sg.nv} vertices; "
                         "timed on rank 0's host cores while the other ranks wait")
            del sg
            torch.cuda.empty_cache()
            return rec

        def strong_check(comm, bounds):  # the strong case against the oracle's run on the bench graph (the N = 1 bench's own run)
            def graph_fn():
                import numpy as np
                from oracle import binding as orc

                sg = synth.make("ogbn-products", seed=42, device="cuda", scale=args.scale)
                rp, ci = sg.rowptr.cpu().numpy(), sg.colidx.cpu().numpy().view(np.uint32)
                del sg
                torch.cuda.empty_cache()
                return orc.Graph(rp, ci).add_selfloop()  # net.cpp:96

            return DistOracleCheck(torch, dist, synth, L, gdist, ctx, comm, args, rank, world, "ogbn-products", (world - 1) / world,
                                   bounds=bounds, graph_fn=graph_fn)

        def parity_at(shape, cut, comm, scale, boundary="uniform"):  # the budgeted parity legs of a default N > 1 run
            a2 = argparse.Namespace(**{**vars(args), "scale": scale})
            return DistOracleCheck(torch, dist, synth, L, gdist, ctx, comm, a2, rank, world, shape, cut, boundary=boundary)

        try:
            if args.workload == "gat-reddit":  # config 4's layer across ranks (round 6; BASELINE pins the config itself to one GPU)
                result = gdist.bench_gat_layer(ctx, args, rank, world, log, hold=hold)
            else:
                result = gdist.bench_gcn_layer(ctx, args, rank, world, D, log, make_check=make_check, t_start=T_START, hold=hold,
                                               cpu_leg=None if args.no_cpu_baseline else cpu_leg,
                                               parity_check=None if (args.no_parity or args.check_oracle) else parity_at,
                                               traffic_of=traffic_from_profile,
                                               strong_check=None if args.no_parity else strong_check)
            dist.barrier()
        except Exception as e:  # noqa: BLE001 -- a sub-case that fails (out of memory, a transport error) after the headline case
            import traceback

            log(f"[bench r{rank}] {type(e).__name__} in the N > 1 leg:\n{traceback.format_exc()}")
            # rank 0: print the record it holds (marked partial; parity = {ok: null, reason} if the comparison had not completed);
            # the others: leave, the launcher ends the job
            guard.bail(f"{type(e).__name__}: {e}"[:300])
            raise
        rc = 0
        if rank == 0:
            cfg = result["config"]
            cfg["launcher"] = launcher
            # a record that says RCCL must have been carried by all N ranks (never a silent subset)
            if cfg["transport"].startswith("gaib_comm/rccl") and cfg.get("rccl_ranks", world) != world:
                log(f"[bench] transport {cfg['transport']} but rccl_ranks = {cfg['rccl_ranks']} != {world}")
                rc = 4
            if result.get("parity") is not None and result["parity"].get("ok") is False:
                log("[bench] PARITY FAILED (> 1e-4)")
                rc = 3
            guard.final(result)
        dist.destroy_process_group()
        if rc:
            sys.exit(rc)
        return

    if args.workload in EPOCH_WORKLOADS:
        try:
            rc = bench_epoch(args, torch, synth, guard)
        except Exception as e:  # noqa: BLE001 -- after the GPU measurement the record is held: print it
            import traceback

            log(f"[bench] {type(e).__name__} in the epoch line:\n{traceback.format_exc()}")
            if guard.held is not None:
                guard.bail(f"{type(e).__name__}: {e}"[:300])
            raise
        if rc:
            sys.exit(rc)
        return

    if args.workload == "gat-reddit":
        try:
            rc = bench_gat_reddit(args, torch, ctx, L, synth, guard)
        except Exception as e:  # noqa: BLE001 -- after the GPU measurement the record is held: print it
            import traceback

            log(f"[bench] {type(e).__name__} in the GAT line:\n{traceback.format_exc()}")
            if guard.held is not None:
                guard.bail(f"{type(e).__name__}: {e}"[:300])
            raise
        if rc:
            sys.exit(rc)
        return

    # ---------------- single GPU -----------------------------------------------------------------
    t0 = time.time()
    sg = synth.make("ogbn-products", seed=42, device="cuda", scale=args.scale)
    torch.cuda.synchronize()
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g1 = g0.add_selfloop()  # GCN aggregates over A + I (net.cpp:96)
    g0.close()
    ctx.sync()
    nv, ne = g1.nv, g1.ne
    stats = ctx.graph_stats(g1)
    log(f"[bench] products-shaped graph: nv={nv} ne={ne} (incl. self loops) max_deg={stats['max_degree']} "
        f"heavy rows={stats['n_heavy']} holding {stats['heavy_edges']} edges; gen+upload {time.time()-t0:.1f}s")
    lg = L.LGraph.adopt(g1)
    want_parity = args.full and not (args.no_cpu_baseline or args.no_parity)
    guard.want_parity = want_parity
    layer = L.Layer(L.GCN, 1, nv, D, D, lg, act=True, lr=0.01)
    if want_parity:
        x_h, gin_h = host_inputs(nv)  # one set of inputs for both legs (element-wise parity below)
        x_d, gin_d = torch.from_numpy(x_h).cuda(), torch.from_numpy(gin_h).cuda()
    else:
        torch.manual_seed(43)
        x_h = gin_h = None
        x_d, gin_d = torch.randn(nv, D, device="cuda"), torch.randn(nv, D, device="cuda")
    layer.write(L.FEAT_IN, x_d)
    layer.write(L.GRAD_IN, gin_d)
    del x_d, gin_d
    feat_out = torch.empty(nv, D, device="cuda")
    grad_out = torch.empty(nv, D, device="cuda")

    def step():
        layer.forward(feat_out)
        layer.backward(feat_out, grad_out)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ctx.prof_reset()
    ctx.prof_enable(True)
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    ctx.prof_enable(False)
    n_light, ms_light = ctx.prof_get("spmm_light")
    n_heavy, ms_heavy = ctx.prof_get("spmm_heavy")
    n_gemm, ms_gemm = ctx.prof_get("sgemm")
    n_fused, ms_fused = ctx.prof_get("spmm_gemm_fused")
    ctx.prof_reset()
    ms_per_step = elapsed / args.steps * 1e3
    if args.dump_outputs:  # before anything else runs the step again
        dump_outputs(Path(args.dump_outputs), torch, L, layer, feat_out, grad_out)

    # sustained leg (not the reported value): the same step for >= --sustain-s seconds, to show the timed figure
    # survives seconds of load (clocks / power); the clocks are sampled mid-run by a child process
    sustained = None
    if args.full and args.sustain_s > 0:
        n_sus = max(int(args.sustain_s * 1e3 / ms_per_step) + 1, args.steps)
        clocks = {}
        th = threading.Thread(target=_sample_clocks, args=(clocks, min(2.0, args.sustain_s / 2)), daemon=True)
        th.start()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(n_sus):
            step()
        torch.cuda.synchronize()
        t_sus = time.perf_counter() - t1
        th.join(timeout=20)
        sustained = {"steps": n_sus, "seconds": t_sus, "ms_per_step": t_sus / n_sus * 1e3,
                     "vs_timed": (t_sus / n_sus * 1e3) / ms_per_step, "clocks_mid_run": clocks or None}

    # the chip's achievable streaming rate, measured in this run: 1 GiB float4 copy, read + written bytes
    peak_measured = ctx.probe_stream_copy(1 << 30, 20) if args.full and args.scale >= 0.05 else None

    edges_per_step = 2 * ne
    value = edges_per_step * args.steps / elapsed
    # algorithmic bytes of ONE launch of the dominant kernel (light rows of one SpMM), SURVEY 8d:
    #   E*(4D + 4 colidx + 4 per-edge weight) + N*4D written + (N+1)*8 rowptr
    e_light = ne - stats["heavy_edges"]
    n_light_rows = nv - stats["n_heavy"]
    if n_fused > 0:
        # the layer's two aggregations run as spmm_gemm_kernel (dense product fused in): per launch the same
        # gathers + the rows it stores -- forward: A.X and the layer output, backward: the input gradient
        # (average 1.5 N x D matrices; the heavy rows' aggregates and the 64 KB of W are noise)
        kernel_name = "spmm_gemm_kernel<VEC=2,edge-weights,U=16,buffer> (aggregation + MFMA dense product)"
        traffic_key = "spmm_gemm_kernel_bytes_per_launch"
        alg_bytes = e_light * (4 * D + 4 + 4) + int(1.5 * nv * 4 * D) + (nv + 1) * 8
        n_dom, ms_dom = n_fused, ms_fused
    else:
        kernel_name = "spmm_w64_kernel<VEC=2,CT=1,edge-weights,U=16,buffer>"
        traffic_key = "spmm_w64_kernel_bytes_per_launch"
        alg_bytes = e_light * (4 * D + 4 + 4) + n_light_rows * 4 * D + (nv + 1) * 8
        n_dom, ms_dom = n_light, ms_light
    avg_ms = ms_dom / max(n_dom, 1)
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9
    # `traffic`: PMC counters need their own rocprofv3 passes (scripts/profile_round.sh: FETCH_SIZE and WRITE_SIZE
    # separately, gfx950 half-count correction), so the per-launch figure comes from the committed summary of the
    # same command -- checked against the kernel sources of THIS tree, dropped on any difference
    traffic, traffic_src = traffic_from_profile(traffic_key) if args.scale == 1.0 else (None, "scale != 1")
    b_min = 2 * nv * 4 * D + 4 * ne
    result = {
        "metric": "GCN-layer fwd+bwd aggregated edges/sec",
        "value": value,
        "unit": "edges/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        # the N > 1 runs partition THIS graph N ways (north_star's curve): total work fixed as N grows
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": "ogbn-products-shaped Chung-Lu graph (seed 42), GCN hidden layer 128->128 fwd+bwd "
                        "(2 SpMM D=128 + 3 dense products + relu/d_relu; 2 of the products ride on the SpMMs)",
            "nv": nv, "ne_with_selfloops": ne, "D": D, "scale": args.scale,
            "parallelism": "1 GPU",
        },
        "roofline": {
            "bound": "hbm", "kernel": kernel_name,
            # achieved = ALGORITHMIC bytes / launch time: every gathered row counted as if it came from HBM.  Part of
            # the gathers hit the 256 MB Infinity Cache, so this can exceed what HBM alone delivers (see
            # peak_measured / frac_of_measured): it is a work rate in bytes, not a physical HBM rate.
            "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            # the same with SURVEY 8(d)'s formula to the letter: ONE N x 4D store per launch (the fused kernel's second
            # stored matrix -- forward keeps A.X for the weight gradient -- not counted)
            "frac_strict_8d": (alg_bytes - (int(1.5 * nv * 4 * D) - nv * 4 * D if n_fused > 0 else 0)) / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "peak_measured": peak_measured,  # stream copy in this run, read + written bytes per second
            "frac_of_measured": (achieved / peak_measured) if peak_measured else None,
            "traffic": traffic, "traffic_source": traffic_src,
            "alg_bytes_per_launch": alg_bytes, "avg_launch_ms": avg_ms, "launches": n_dom,
            # perfect-reuse lower bound of one aggregation (every feature row read once) and how far the
            # measured L2->fabric traffic is above it (no reuse of gathered rows in a 4 MB L2 on a random vertex order)
            "b_min_bytes_per_launch": b_min,
            "traffic_over_b_min": (traffic / b_min) if traffic else None,
            # FETCH_SIZE x2 + WRITE_SIZE per launch time over the spec peak: L2 -> fabric bytes, Infinity-Cache hits
            # INCLUDED (MI355X_MICROARCH.md), i.e. an upper bound on the HBM share, not an HBM measurement
            "fabric_traffic_frac": (traffic / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic else None,
        },
        # the aggregation kernels alone (both SpMM launches of the step incl. heavy rows; the dense products that
        # ride on them are inside): aggregated edges per second of kernel time
        "aggregation_only_edges_per_s": edges_per_step * args.steps / max((ms_fused + ms_light + ms_heavy) * 1e-3, 1e-9),
        "breakdown_ms_per_step": {
            "spmm_gemm_fused": ms_fused / args.steps, "spmm_light": ms_light / args.steps,
            "spmm_heavy": ms_heavy / args.steps, "sgemm": ms_gemm / args.steps,
        },
    }
    if sustained:
        result["sustained_ms_per_step"] = sustained["ms_per_step"]
        result["sustained"] = sustained
    # The bench graph's vertex ids are randomly permuted ON PURPOSE (no locality: traffic / b_min = 19).  Beside it, the
    # same kernel on a graph of the same shape whose numbering carries locality (planted communities of 16 384 consecutive
    # ids, 10 % of a vertex's edges leave its community): what the XCD-affine tile supply and the L2s are worth when the
    # numbering offers something.  Not part of `value`.
    # The GPU measurement is complete.  What follows -- the locality leg, the CPU baseline, the comparison with the oracle -- only
    # adds to the record: it is HELD from here on (RecordGuard, as in the N > 1 leg) and printed, marked partial, if a signal, the
    # deadline or an exception in one of those legs ends the run first.
    guard1 = guard  # (installed first thing in main(); its deadline counts from the process's start)
    guard1.hold(result)
    rc = 0
    try:
        if args.full and args.scale == 1.0 and not args.no_locality and os.environ.get("GAIB_BENCH_LOCALITY", "1") != "0":
            try:
                result["roofline"]["planted_locality"] = locality_leg(torch, ctx, capi, synth)
            except Exception as e:  # noqa: BLE001 -- a side measurement must not cost the headline record
                result["roofline"]["planted_locality"] = {"error": f"{type(e).__name__}: {e}"[:200]}
        if os.environ.get("GAIB_BENCH_FAIL_AFTER_HEADLINE") == "0":  # test hook (tests/test_gpu_dist.py)
            raise RuntimeError("GAIB_BENCH_FAIL_AFTER_HEADLINE: injected failure after the GPU measurement")
        if args.full and not args.no_cpu_baseline:
            t1 = time.time()
            xs = (x_h, gin_h) if want_parity else host_inputs(nv)
            result["cpu_baseline"], want = cpu_baseline(sg.rowptr, sg.colidx, nv, *xs, want_outputs=want_parity)
            log(f"[bench] cpu baseline took {time.time()-t1:.1f}s")
            if want_parity:
                gview = lg.device_graph()  # (non-owning view of the layer's graph; the copies of its arrays need the context)
                gview.ctx = ctx
                result["parity"] = parity_record(torch, L, layer, feat_out, grad_out, gin_h, want, graph=gview,
                                                 feat_in=layer.tensor(L.FEAT_IN, (nv, D)))
                log(f"[bench] parity vs the oracle's full-graph run: {result['parity']}")
                if not result["parity"]["ok"]:
                    log("[bench] PARITY FAILED (> 1e-4)")
                    rc = 3
        # ---- BASELINE configs 2-4 in the --full run: after everything the headline
        # record needs -- its value, roofline, CPU baseline and parity are complete and held; this block only adds a slot
        if args.full and args.other_configs_s > 0 and os.environ.get("GAIB_BENCH_OTHER_CONFIGS", "1") != "0":
            layer.close()
            lg.close()
            del feat_out, grad_out
            torch.cuda.empty_cache()
            # (the block's own budget, and never past the run's deadline: 25 s are left for the last leg to be cut and the record to leave)
            t_end = min(time.time() + args.other_configs_s, T_START + args.deadline_s - 25.0)

            def upd(o):
                result["other_configs"] = o
                guard1.hold(result)

            other_configs(args, torch, ctx, L, synth, sg, t_end, upd)
    except Exception as e:  # noqa: BLE001
        import traceback

        log(f"[bench] {type(e).__name__} after the GPU measurement:\n{traceback.format_exc()}")
        guard1.bail(f"{type(e).__name__}: {e}"[:300])  # prints the held record, marked partial, parity = {ok: null, reason}
        raise
    guard1.final(result)
    if rc:
        sys.exit(rc)


def locality_leg(torch, ctx, capi, synth, reps: int = 6) -> dict:
    """the fused aggregation + product kernel (the headline's dominant kernel) on the planted-locality graph"""
    sg = synth.planted_locality("ogbn-products", 16384, 0.1, seed=42, device="cuda")
    g = ctx.graph(sg.rowptr, sg.colidx)
    nv, ne = g.nv, g.ne
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    x = torch.randn(nv, D, device="cuda", generator=gen)
    W = torch.randn(D, D, device="cuda", generator=gen) * 0.1
    agg, y = torch.empty_like(x), torch.empty_like(x)
    ctx.spmm_gemm(g, capi.W_GCN, x, agg, W, y)
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    for _ in range(reps):
        ctx.spmm_gemm(g, capi.W_GCN, x, agg, W, y)
    ctx.prof_enable(False)
    n, ms = ctx.prof_get("spmm_gemm_fused")
    st = ctx.graph_stats(g)
    ctx.prof_reset()
    avg_ms = ms / max(n, 1)
    alg = (ne - st["heavy_edges"]) * (4 * D + 8) + 2 * nv * 4 * D + (nv + 1) * 8
    b_min = 2 * nv * 4 * D + 4 * ne
    traffic, src = traffic_from_profile("spmm_gemm_kernel_bytes_per_launch", "planted_locality")
    g.close()
    fabric = (traffic / (avg_ms * 1e-3) / 1e9) if traffic else None
    return {"graph": sg.name, "nv": nv, "ne_with_selfloops": ne, "kernel_ms": avg_ms,
            # algorithmic rate: every gathered row counted -- here most of them are L2 / Infinity-Cache hits, so this is a work
            # rate above any memory peak, NOT a roofline fraction; `frac` prices the L2 -> fabric bytes (PMC) instead
            "algorithmic_gbs": alg / (avg_ms * 1e-3) / 1e9, "alg_bytes_per_launch": alg,
            "fabric_gbs": fabric, "frac": (fabric / HBM_PEAK_GBS) if fabric else None, "peak": HBM_PEAK_GBS,
            "b_min_bytes_per_launch": b_min, "traffic": traffic, "traffic_source": src,
            "traffic_over_b_min": (traffic / b_min) if traffic else None}


def bench_gat_reddit(args, torch, ctx, L, synth, guard) -> int:
    """BASELINE config 4 ("reddit GAT 2-layer 8-head", SDDMM + edge-softmax kernel path): the hidden GAT layer 64 -> 64
    with 8 heads (8 x 8 columns), forward + backward per step, on the reddit-shaped graph with self loops (net.cpp:96).
    `value` = aggregated edges per second (2 attention-weighted aggregations per step).  The table (60 MB) lives in the
    Infinity Cache, so the roofline record prices the dominant kernel against the 8 TB/s HBM peak AND the guide's
    cache-resident gather rate.  cpu_baseline: the oracle's GAT layer for the first `heads_sampled` heads (a head is an
    independent single-head layer over all edges; gat_aggregator.cpp:57-200), same inputs; parity on those heads."""
    import numpy as np

    Dg, H = 64, 8
    t0 = time.time()
    sg = synth.make("reddit", seed=7, device="cuda", scale=args.scale)
    g0 = ctx.graph(sg.rowptr, sg.colidx)
    g1 = g0.add_selfloop()
    g0.close()
    ctx.sync()
    nv, ne = g1.nv, g1.ne
    log(f"[bench] reddit-shaped graph: nv={nv} ne={ne} (incl. self loops); gen+upload {time.time()-t0:.1f}s")
    lg = L.LGraph.adopt(g1)
    rng = np.random.default_rng(43)
    x_h = rng.standard_normal((nv, Dg), dtype=np.float32)
    gin_h = rng.standard_normal((nv, Dg), dtype=np.float32)
    layer = L.Layer(L.GAT, 1, nv, Dg, Dg, lg, act=True, lr=0.01)
    layer.set_heads(H)
    layer.write(L.FEAT_IN, torch.from_numpy(x_h).cuda())
    gin_d = torch.from_numpy(gin_h).cuda()
    layer.write(L.GRAD_IN, gin_d)
    feat_out = torch.empty(nv, Dg, device="cuda")
    grad_out = torch.empty(nv, Dg, device="cuda")

    def step():
        layer.forward(feat_out)
        layer.backward(feat_out, grad_out)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ctx.prof_reset()
    ctx.prof_enable(True)
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    ctx.prof_enable(False)
    keys = ["gat_vertex_dots", "gat_edge_softmax", "gat_fwd_fused", "gat_bwd_fused", "gat_sddmm", "gat_softmax_bwd_alpha", "spmm_chunk", "spmm_chunk_reduce",
            "spmm_light", "spmm_heavy", "spmm_gemm_fused", "sgemm", "relu", "d_relu"]
    prof = {}
    for k in keys:
        n, ms = ctx.prof_get(k)
        if n:
            prof[k] = (n, ms)
    ctx.prof_reset()
    ms_per_step = elapsed / args.steps * 1e3
    sustained = None
    if args.sustain_s > 0:
        n_sus = max(int(args.sustain_s * 1e3 / ms_per_step) + 1, args.steps)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(n_sus):
            step()
        torch.cuda.synchronize()
        sustained = (time.perf_counter() - t1) / n_sus * 1e3
    peak_measured = ctx.probe_stream_copy(1 << 30, 20) if args.scale >= 0.05 else None
    # ALGORITHMIC bytes per launch of the per-edge kernels: records are 4*H bytes per edge and array
    alg = {
        "gat_edge_softmax": ne * (4 + 4 * H + 4 * H) + nv * 8 * H,             # col + gathered dot + attention written
        "gat_sddmm": ne * (4 + 4 * Dg + 4 * H) + nv * 4 * Dg,                    # col + gathered row + dp written
        "gat_softmax_bwd_alpha": ne * (4 + 4 + 3 * 4 * H) + nv * (2 * 4 * Dg),  # col, rev, p, dp read, p^T written
        "spmm_chunk": ne * (4 + 4 * Dg + 4 * H) + (ne // 64) * 4 * Dg,          # col + gathered row + weights, partial rows
        # the fused edge side of backward: col, rev, p_e, p_rev, rowdot of the column vertex and TWO gathered rows per edge
        # (h_c, grad_c); partial rows per chunk written and read once; nothing per edge is written
        # (with the one-sweep forward the attention is formed again from row statistics: 8 B per (edge, head) of stats
        # instead of p_e, p_rev and rev)
        "gat_bwd_fused": ne * (4 + 2 * 4 * H + 2 * 4 * Dg + 4 * H) + (ne // 64) * (4 * Dg + 8 * H) * 2,
        # one-sweep forward: col + ONE gathered row per edge; partial rows and (max, sum) per chunk written and read once
        "gat_fwd_fused": ne * (4 + 4 * Dg) + (ne // 64) * (4 * Dg + 8 * H) * 2 + nv * (4 * Dg + 8 * H),
    }
    dom = max((k for k in prof if k in alg), key=lambda k: prof[k][1], default=None)
    roof = None
    if dom:
        n_dom, ms_dom = prof[dom]
        avg_ms = ms_dom / n_dom
        ach = alg[dom] / (avg_ms * 1e-3) / 1e9
        # `traffic`: like the GCN line, from the committed PMC summary of this command (separate rocprofv3 passes),
        # verified against this tree's kernel sources
        traffic, traffic_src = traffic_from_profile(f"{dom}_bytes_per_launch", "gat_reddit") if args.scale == 1.0 else (None, "scale != 1")
        # What bounds this kernel: the 60 MB feature table lives in the 256 MB Infinity Cache, the 4 MB L2s filter part
        # of the gathers, and what is left crosses the fabric at the cache-resident gather rate -- MI355X_MICROARCH.md
        # measures 8.6 TB/s for a table of this size gathered uniformly.  `frac` = (L2 -> fabric bytes per launch, PMC) /
        # launch time / that rate.  The algorithmic rate (every gathered row counted, L2 hits included) exceeds any
        # memory peak and is reported beside it, NOT as a roofline fraction.
        CACHE_GATHER_GBS = 8600.0
        fabric = (traffic / (avg_ms * 1e-3) / 1e9) if traffic else None
        roof = {"bound": "infinity-cache gather", "kernel": dom, "achieved": fabric, "peak": CACHE_GATHER_GBS, "unit": "GB/s",
                "frac": (fabric / CACHE_GATHER_GBS) if fabric else None,
                "traffic": traffic, "traffic_source": traffic_src,
                "algorithmic_gbs": ach, "alg_bytes_per_launch": alg[dom],
                # L2 -> fabric bytes per launch over the algorithmic bytes: what the 4 MB L2s filter out of the gathers
                "traffic_over_alg": (traffic / alg[dom]) if traffic else None,
                "hbm_peak": HBM_PEAK_GBS, "peak_measured_stream_copy": peak_measured,
                "avg_launch_ms": avg_ms, "launches": n_dom}
    result = {
        "metric": "GAT-layer fwd+bwd aggregated edges/sec", "value": 2 * ne * args.steps / elapsed, "unit": "edges/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "reddit-shaped Chung-Lu graph (seed 7), GAT hidden layer 64->64 with 8 heads fwd+bwd "
                               "(X.W, per-vertex dots, edge softmax, 2 attention SpMM, SDDMM, softmax backward + alpha "
                               "gradients + transpose, 2 weight-side GEMMs)",
                   "nv": nv, "ne_with_selfloops": ne, "D": Dg, "heads": H, "scale": args.scale, "parallelism": "1 GPU"},
        "roofline": roof,
        "breakdown_ms_per_step": {k: v[1] / args.steps for k, v in prof.items()},
    }
    if sustained:
        result["sustained_ms_per_step"] = sustained
    # the GPU measurement is complete: the record is held from here on (as in the GCN line; main() bails on an exception)
    guard.hold(result)
    rc = 0
    if not args.no_cpu_baseline:
        from oracle import binding as orc

        cores = usable_cores()
        orc.set_threads(cores)
        dh = Dg // H
        g_o = orc.Graph(sg.rowptr.cpu().numpy(), sg.colidx.cpu().numpy().view(np.uint32)).add_selfloop()
        W = orc.init_glorot(Dg, Dg, 1)
        al, ar = orc.init_glorot(Dg, 1, 2).ravel(), orc.init_glorot(Dg, 1, 3).ravel()
        hfeat = orc.matmul(x_h, W)
        # ALL heads (a head is an independent single-head layer over all edges, gat_aggregator.cpp:57-200): ~10 s on
        # the box's cores, and the whole layer -- forward, input gradient, weight gradient, alpha gradients -- becomes
        # comparable element by element (round 2 sampled 2 heads and compared the forward only)
        t1 = time.perf_counter()
        outs, temps, norms = [], [], []
        for k in range(H):
            sl = slice(k * dh, (k + 1) * dh)
            o, t, _, p_ = orc.gat_aggregate(g_o, np.ascontiguousarray(hfeat[:, sl]), np.ascontiguousarray(al[sl]),
                                            np.ascontiguousarray(ar[sl]))
            outs.append(np.maximum(o, 0))
            temps.append(t)
            norms.append(p_)
        want = np.concatenate(outs, 1)
        g_act = np.where(want > 0, gin_h, 0).astype(np.float32)
        T = np.empty((nv, Dg), np.float32)
        lg_w, rg_w = np.empty(Dg, np.float32), np.empty(Dg, np.float32)
        for k in range(H):
            sl = slice(k * dh, (k + 1) * dh)
            go, _, _, l_, r_ = orc.gat_d_aggregate(g_o, np.ascontiguousarray(hfeat[:, sl]), np.ascontiguousarray(g_act[:, sl]),
                                                   norms[k], temps[k], fast=True)
            T[:, sl], lg_w[sl], rg_w[sl] = go, l_, r_
        t_cpu = time.perf_counter() - t1
        result["cpu_baseline"] = dict(value=2 * ne / t_cpu, unit="edges/s", cores=cores, cores_available=os.cpu_count(),
                                      kind="port",
                                      sample=f"all {H} attention heads over the whole graph ({ne} edges incl. self loops), score + "
                                             f"softmax + aggregation forward and backward (`fast` d_softmax), {t_cpu:.2f} s "
                                             f"(the dense products X.W, T.W^T, X^T.T of the layer are outside the timed CPU region)")
        want_go = orc.matmul(T, W, False, True)
        want_wg = orc.matmul(x_h, T, True, False)
        del norms, outs
        # parity, as in parity_record: forward as is; backward re-run on the ORACLE's forward output (identical relu masks)
        tol, floor = 1e-4, 1e-5  # rows of up to 21 k edges, K = 233 k weight gradient: long-sum floor (tests/util.py)
        layer.write(L.GRAD_IN, gin_d)
        layer.forward(feat_out)
        torch.cuda.synchronize()
        want_d = torch.from_numpy(want).cuda()
        par = {"tol": tol, "floor_frac_of_max": floor, "heads_compared": H,
               "forward": _errs(torch, feat_out, want_d, tol, floor)}
        flips = (feat_out > 0) != (want_d > 0)
        par["relu_mask_flips"] = {"count": int(flips.sum().item()), "of": int(want_d.numel())}
        layer.write(L.GRAD_IN, gin_d)
        layer.backward(want_d, grad_out)
        torch.cuda.synchronize()
        par["grad_out"] = _errs(torch, grad_out, torch.from_numpy(want_go).cuda(), tol, floor)
        par["W_grad"] = _errs(torch, layer.tensor(L.W_NEIGH_GRAD, (Dg, Dg)), torch.from_numpy(want_wg).cuda(), tol, floor)
        # alpha gradients: 64 sums over 9e8 (edge, head) terms with leaky_relu' jumping at 0 -- a score within rounding of
        # zero takes either slope in two correct fp32 evaluations, and ~15 such flips are worth ~1e-4 of the largest
        # entry.  So arithmetic is compared the way backward is compared on the oracle's relu mask: the signs each
        # implementation takes (the GPU's: gaib_gat_score_signs, the kernels' exact arithmetic) are imposed on an fp64
        # evaluation of the same formulas on the device (oracle/fp64.py), and each is held to 1e-4 of ITS fp64 counterpart
        from oracle import fp64 as truth
        # (the GPU's own h = X.W, by the product kernel the layer runs: it differs from the oracle's h in the last place,
        # which is enough to move a score across zero)
        h_gpu = torch.empty(nv, Dg, device="cuda")
        ctx.sgemm(torch.from_numpy(x_h).cuda(), torch.from_numpy(W).cuda(), h_gpu)
        ctx.sync()
        signs_gpu = ctx.gat_score_signs(lg.device_graph(), h_gpu, torch.from_numpy(al).cuda(), torch.from_numpy(ar).cuda(), heads=H)
        signs_orc = torch.from_numpy(np.stack(temps, 1) > 0).cuda().to(torch.uint8)
        par["leaky_relu_signs_gpu_vs_oracle_differ"] = int((signs_gpu != signs_orc).sum().item())
        lg_g64, rg_g64, info = truth.gat_alpha_grads_fp64(g_o.rowptr, g_o.colidx, h_gpu, al, ar, g_act, H, signs=signs_gpu)
        del h_gpu
        lg_o64, rg_o64, info_o = truth.gat_alpha_grads_fp64(g_o.rowptr, g_o.colidx, hfeat, al, ar, g_act, H, signs=signs_orc)
        ok_a = info["imposed_flips_max_abs_t_over_scale"] < 1e-5 and info_o["imposed_flips_max_abs_t_over_scale"] < 1e-5
        for which, want_a, g64, o64, name in ((L.ALPHA_LGRAD, lg_w, lg_g64, lg_o64, "alpha_l_grad"),
                                              (L.ALPHA_RGRAD, rg_w, rg_g64, rg_o64, "alpha_r_grad")):
            got = layer.tensor(which, (Dg,)).double().cpu().numpy()
            rec_a = {"inf_vs_fp64_on_own_signs": truth.inf_dist(got, g64),
                     "oracle_inf_vs_fp64_on_own_signs": truth.inf_dist(want_a, o64),
                     "inf_vs_oracle_as_they_are": truth.inf_dist(got, want_a)}
            ok_a = ok_a and rec_a["inf_vs_fp64_on_own_signs"] <= tol and rec_a["oracle_inf_vs_fp64_on_own_signs"] <= tol
            par[name] = rec_a
        par["leaky_relu_sign_flips_vs_fp64"] = {"gpu": info["imposed_sign_flips_vs_fp64"], "oracle": info_o["imposed_sign_flips_vs_fp64"],
                                                "max_abs_score_over_scale": max(info["imposed_flips_max_abs_t_over_scale"],
                                                                                info_o["imposed_flips_max_abs_t_over_scale"])}
        par["ok"] = bool(all(par[k]["elem"] <= tol and par[k]["inf"] <= tol for k in ("forward", "grad_out", "W_grad")) and ok_a)
        result["parity"] = par
        log(f"[bench] parity vs the oracle's {H}-head run: {par}")
        if not par["ok"]:
            log("[bench] PARITY FAILED (> 1e-4)")
            rc = 3
    layer.close()
    lg.close()
    del feat_out, grad_out, gin_d
    torch.cuda.empty_cache()
    guard.final(result)
    return rc


# ---- the other BASELINE configs inside the N = 1 run with --full --------------------------------------------
class _Capture:
    """stands in for the RecordGuard where a leg's record goes into a slot of the --full run's record instead of out"""
    held = None

    def hold(self, r):
        self.held = r

    final = hold


def sage_layer_step(torch, ctx, L, sg, width: int, steps: int, warmup: int) -> dict:
    """BASELINE config 3's layer: one GraphSAGE hidden layer width -> width forward + backward on the products-shaped graph
    (A without self loops, net.cpp:96) -- two mean aggregations with the neighbour product riding on them, the self products,
    the two weight gradients -- with the per-launch work table priced at the chip's roofs (as the epoch records do)"""
    g = ctx.graph(sg.rowptr, sg.colidx)
    nv, ne = g.nv, g.ne
    lg = L.LGraph.adopt(g)
    layer = L.Layer(L.SAGE, 1, nv, width, width, lg, act=True, lr=0.01)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(43)
    layer.write(L.FEAT_IN, torch.randn(nv, width, device="cuda", generator=gen))
    layer.write(L.GRAD_IN, torch.randn(nv, width, device="cuda", generator=gen))
    fo, go = torch.empty(nv, width, device="cuda"), torch.empty(nv, width, device="cuda")

    def step():
        layer.forward(fo)
        layer.backward(fo, go)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ctx.prof_reset()
    ctx.prof_enable(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ctx.prof_enable(False)
    table = ctx.prof_table()
    ctx.prof_reset()
    layer.close()
    lg.close()
    del fo, go
    torch.cuda.empty_cache()
    ms = el / steps * 1e3
    roof = sum(v["roof_ms"] for v in table.values()) / steps
    dom = max(table, key=lambda k: table[k]["ms"]) if table else None
    return {"workload": f"GraphSAGE hidden layer {width} -> {width} fwd+bwd on the ogbn-products-shaped graph (seed 42, no self loops)",
            "value": 2 * ne * steps / el, "unit": "edges/s", "ms_per_step": ms, "steps": steps, "warmup": warmup, "nv": nv, "ne": ne,
            "roofline": {"frac": roof / ms, "frac_definition": "sum over the step's launches of max(algorithmic bytes / 8 TB/s, flops / 157.3 TFLOP/s), "
                         "over the measured step time", "roof_ms_per_step": roof,
                         "largest": dom, "per_key": {k: {"ms_per_step": v["ms"] / steps, "frac": (v["roof_ms"] / v["ms"]) if v["ms"] > 0 else None}
                                                     for k, v in sorted(table.items(), key=lambda kv: -kv[1]["ms"])[:6]}}}


def _brief_epoch(r: dict) -> dict:
    """an epoch record cut down to what a slot of other_configs carries (the full one: `bench.py --workload epoch-*`)"""
    pk = r["roofline"]["per_key"]
    top = sorted(pk, key=lambda k: -pk[k]["ms_per_epoch"])[:8]
    return {"workload": r["config"]["workload"], "value": r["value"], "unit": r["unit"], "ms_per_epoch": r["ms_per_step"], "steps": r["steps"],
            "warmup": r["warmup"], "nv": r["config"]["nv"], "ne": r["config"]["ne"], "hidden": r["config"]["hidden"],
            "aggregated_edges_per_epoch": r["config"]["aggregated_edges_per_epoch"], "recorded_epochs": bool(r["config"]["recorded_epochs"]),
            "train_loss_timed_epochs": r["config"]["train_loss_timed_epochs"],
            "roofline": {"frac": r["roofline"]["frac"], "frac_definition": r["roofline"]["frac_definition"],
                         "roof_ms_per_epoch": r["roofline"]["roof_ms_per_epoch"], "untimed_ms_per_epoch": r["roofline"]["untimed_ms_per_epoch"],
                         "frac_note": r["roofline"].get("frac_note"),
                         "per_key": {k: {"ms_per_epoch": pk[k]["ms_per_epoch"], "frac": pk[k]["frac"],
                                         **({"frac_of_line_floor": pk[k]["line_floor"]["frac_of_line_floor"]} if "line_floor" in pk[k] else {})}
                                     for k in top}}}


def other_configs(args, torch, ctx, L, synth, sg, t_budget_end: float, on_update) -> dict:
    """BASELINE configs 2-4 as short legs of the DEFAULT run, after the headline record is held -- so that the driver's own
    `bench.py --gpus 1` witnesses them (round 5: everything but the headline was builder-run): the SAGE layer step at 128 and
    256, the 8-head GAT layer on the reddit shape, and the epoch workloads through the trainer CLI (10 timed epochs each; the
    products dataset written once for the three models on it).  Every leg is budgeted -- it starts only if its estimated time
    fits what is left of --other-configs-s -- and failure-proof: a slot says {"skipped": ...} or {"error": ...}, the headline
    `value` and its timed region are long done.  GPU timings only (no CPU baseline, no parity: the per-workload commands have them)."""
    import argparse
    import shutil
    import tempfile

    out = {"budget_s": args.other_configs_s}
    t_block = time.time()

    def leg(name, need_s, fn):
        left = t_budget_end - time.time()
        if left < need_s:
            out[name] = {"skipped": "budget", "needed_s_estimate": need_s, "left_s": round(left, 1)}
        else:
            t0 = time.time()
            try:
                out[name] = fn()
                out[name]["leg_seconds"] = round(time.time() - t0, 1)
            except Exception as e:  # noqa: BLE001 -- a side leg must not cost the record
                import traceback

                log(f"[bench] other_configs.{name}: {type(e).__name__}:\n{traceback.format_exc()}")
                out[name] = {"error": f"{type(e).__name__}: {e}"[:300]}
            torch.cuda.empty_cache()
        out["elapsed_s"] = round(time.time() - t_block, 1)
        on_update(out)

    full = args.scale == 1.0
    st = 10
    leg("sage_layer_128", 6 if full else 3, lambda: sage_layer_step(torch, ctx, L, sg, 128, st, 3))
    leg("sage_layer_256", 8 if full else 3, lambda: sage_layer_step(torch, ctx, L, sg, 256, st, 3))

    def gat_layer():
        cap = _Capture()
        a2 = argparse.Namespace(**{**vars(args), "steps": st, "warmup": 3, "sustain_s": 0.0, "no_cpu_baseline": True})
        bench_gat_reddit(a2, torch, ctx, L, synth, cap)
        r = cap.held
        return {"workload": r["config"]["workload"], "value": r["value"], "unit": r["unit"], "ms_per_step": r["ms_per_step"], "steps": st,
                "nv": r["config"]["nv"], "ne": r["config"]["ne_with_selfloops"], "heads": r["config"]["heads"], "roofline": r["roofline"],
                "breakdown_ms_per_step": r["breakdown_ms_per_step"]}

    leg("gat_layer_reddit_8x8", 12 if full else 4, gat_layer)
    why = profiler_preload()
    if why:
        for k in ("epoch_sage_products_hidden256", "epoch_sage_products_hidden128", "epoch_gcn_products", "epoch_gat_reddit", "epoch_gcn_cora"):
            out[k] = {"skipped": f"{why}: the epoch legs start the trainer as a child program (profile bin/gpu_train_* directly)"}
        return out
    ea = argparse.Namespace(**{**vars(args), "steps": st, "warmup": 2, "no_cpu_baseline": True})
    data = tempfile.mkdtemp(prefix="gaib_other_")
    try:
        ep = lambda w, **kw: (lambda: _brief_epoch(epoch_record(ea, torch, synth, wname=w, data_root=data, keep_data=True, **kw)[0]))
        leg("epoch_sage_products_hidden256", 40 if full else 8, ep("epoch-sage-products", hidden=256))
        leg("epoch_sage_products_hidden128", 18 if full else 6, ep("epoch-sage-products", hidden=128))
        leg("epoch_gcn_products", 15 if full else 6, ep("epoch-gcn-products"))
        shutil.rmtree(os.path.join(data, "ogbn-products"), ignore_errors=True)
        leg("epoch_gat_reddit", 30 if full else 8, ep("epoch-gat-reddit"))
        shutil.rmtree(os.path.join(data, "reddit"), ignore_errors=True)
        leg("epoch_gcn_cora", 12, ep("epoch-gcn-cora"))
    finally:
        shutil.rmtree(data, ignore_errors=True)
    return out


# ---- epoch-level records (BASELINE configs 2-4 are models, not layers) ------------------------------------
EPOCH_WORKLOADS = {
    # /root/reference/scripts/run-sage-products.sh:1  `cpu_train_sage ogbn-products 10 32 softmax 256 0 0 0.01 3 0 50 0`
    "epoch-sage-products": dict(arch="sage", dataset="ogbn-products", hidden=256, layers=3, heads=1, parity_scale=0.04,
                                what="BASELINE config 3 as scripted: 3-layer GraphSAGE 100 -> 256 -> 256 -> 47 on the ogbn-products "
                                     "shape (scripts/run-sage-products.sh)"),
    "epoch-gcn-products": dict(arch="gcn", dataset="ogbn-products", hidden=128, layers=3, heads=1, parity_scale=0.04,
                               what="3-layer GCN 100 -> 128 -> 128 -> 47 on the ogbn-products shape (north_star's D = 128 as a model)"),
    # BASELINE config 2: "cora GCN 2-layer D=16 fp32 on 1 MI355X" -- the reference's own topology (tests/golden/cora), seeded features
    "epoch-gcn-cora": dict(arch="gcn", dataset="cora", hidden=16, layers=2, heads=1, parity_scale=1.0,
                           what="BASELINE config 2: 2-layer GCN 1433 -> 16 -> 7 on the cora topology the reference ships (launch-bound: "
                                "the timed epochs are replayed as recorded HIP graphs; the work table comes from a second, "
                                "call-by-call run)"),
    "epoch-gat-reddit": dict(arch="gat", dataset="reddit", hidden=64, layers=2, heads=8, parity_scale=0.1,
                             what="BASELINE config 4: 2-layer 8-head GAT 602 -> 64 -> 64 (+ l2norm + dense 64 -> 41, net.cpp:69-71) "
                                  "on the reddit shape"),
}


def _lines_per_row(cols: int) -> float:
    """128-B lines a gathered row of `cols` floats touches, averaged over rows of a table whose rows are padded to whole
    float4s (the library re-strides odd widths: 47 -> 48 floats = 192 B): the physical floor of a gather, where
    SURVEY 8(d)'s algorithmic figure counts 4 * cols bytes"""
    stride, width = ((cols + 3) // 4) * 16, cols * 4
    n = 0
    for k in range(32):  # the alignment pattern repeats after lcm(stride, 128) / stride <= 32 rows
        a = k * stride
        n += (a + width - 1) // 128 - a // 128 + 1
    return n / 32.0


def _run_trainer(arch: str, data_root: str, dataset: str, epochs: int, hidden: int, layers: int, heads: int, prof_from: int | None,
                 timeout_s: float, times_from: int | None = None):
    """bin/gpu_train_<arch> with the reference's argument list (train.cpp:9-14; net.cpp:40-64) as a CHILD process ->
    (stdout text, per-epoch dicts (loss, acc, seconds), work table or {}, aggregated edges per epoch)"""
    import re

    from graphaibench_amd import capi

    why = profiler_preload()
    if why:  # (as launch_ranks: the tool library has initialised the GPU in THIS process, and the child would be profiled into it)
        raise RuntimeError(f"{why}: the epoch workloads start the trainer as a child program, which a process under a profiler must "
                           "not do on this pool -- profile bin/gpu_train_* directly after `--` (scripts/profile_epoch.sh)")
    exe = ROOT / "bin" / f"gpu_train_{arch}"
    if not exe.exists():
        raise RuntimeError(f"{exe} is missing: python -m graphaibench_amd.build")
    env = dict(os.environ, DATASET_PATH=data_root if data_root.endswith("/") else data_root + "/", GAIB_GAT_HEADS=str(heads))
    env.pop("GAIB_RANKS", None)
    env["GAIB_EPOCH_LOSSES"] = "1"  # train_loss / train_acc once more with 9 digits (the log line keeps the reference's three decimals)
    if times_from is not None:  # epoch times at full precision without timing launches (recorded epochs included)
        env["GAIB_EPOCH_TIMES"] = str(times_from)
    if prof_from is not None:
        env["GAIB_PROF_TABLE"] = str(prof_from)
        # (launch-bound datasets -- <= 4 M edges: cora, scaled-down development runs -- are replayed as recorded HIP graphs, where
        # nothing is launched call by call and no launch can be timed: the table needs a call-by-call run; the full-size
        # configs run call by call anyway)
        env["GAIB_EPOCH_GRAPH"] = "0"
    # <dataset> <epochs> <threads> <loss> <hidden> <score_drop> <feat_drop> <lr> <layers> <subgraph> <val_interval> <inductive>
    cmd = [str(exe), dataset, str(epochs), "32", "softmax", str(hidden), "0", "0", "0.01", str(layers), "0", str(epochs + 100), "0"]
    rcode, r_out, r_err = run_child(cmd, env=env, timeout_s=timeout_s)

    class r:  # (the fields the code below reads)
        returncode, stdout, stderr = rcode, r_out, r_err

    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} exited with {r.returncode}: {r.stderr[-600:]}")
    ep = [dict(loss=float(a), acc=float(b), seconds=float(c))
          for a, b, c in re.findall(r"train_loss ([0-9.]+) train_acc ([0-9.]+) train_time ([0-9.]+) s", r.stdout)]
    for key, field in (("epoch_losses", "loss"), ("epoch_accs", "acc")):  # full precision where the trainer gave it
        mm = re.search(rf"^\[gaib prof\] {key}((?: [0-9.eE+-]+)+)$", r.stdout, re.M)
        if mm and len(mm.group(1).split()) == len(ep):
            for e, v in zip(ep, mm.group(1).split()):
                e[field] = float(v)
    table = capi.parse_prof_table("\n".join(l[len("[gaib prof] "):] for l in r.stdout.splitlines() if l.startswith("[gaib prof] ")))
    m = re.search(r"Aggregated edges per epoch: (\d+)", r.stdout)
    # the profiled epochs' times at full precision (the log line keeps the reference's three decimals: 1 ms)
    ms = re.search(r"^\[gaib prof\] epoch_seconds((?: [0-9.]+)+)$", r.stdout, re.M)
    if ms:
        exact = [float(v) for v in ms.group(1).split()]
        for e, t in zip(ep[len(ep) - len(exact):], exact):
            e["seconds"] = t
    return r.stdout, ep, table, int(m.group(1)) if m else 0


def bench_epoch(args, torch, synth, guard) -> int:
    """`--workload epoch-*`: the record of epoch_record, held as soon as the GPU measurement is in, then printed"""
    result, rc = epoch_record(args, torch, synth, hold=guard.hold, hidden=getattr(args, "hidden", None))
    guard.final(result)
    return rc


def epoch_record(args, torch, synth, hold=None, wname=None, hidden=None, data_root=None, keep_data=False):
    """-> (record, rc).  One training EPOCH of a BASELINE model config per step, through the trainer CLI the reference's scripts call
    (bin/gpu_train_*: reader -> Model -> forward_prop / backward_prop / update, src/gnn/net.cpp:361-419) on a seeded synthetic
    dataset of the config's shape in the reference's on-disk format.  --warmup epochs run first (epoch 0 allocates and builds
    the graph's lazily made tables), then --steps epochs are timed -- the trainer's own per-epoch train_time, each bracketed
    by a device synchronisation.  `value` = aggregated edges per second (edges of the graph x aggregation calls of an epoch).
    roofline: every library launch of the timed epochs states its algorithmic work; `frac` = the time those
    launches would take at the chip's roofs -- per launch max(bytes / 8 TB/s, flops / 157.3 TFLOP/s) -- over the measured
    epoch time; per kernel and row width in `per_key`, with the 128-B-line floor of the gathers whose rows are no whole
    number of lines (D = 47, 100) next to their algorithmic bytes.
    cpu_baseline + parity: the oracle's Model (oracle/model.py) on the same generator at `parity_scale` -- its epoch timed, and the
    first 5 train_loss / train_acc of the trainer on that dataset against it (GAIB_EPOCH_LOSSES: 9 digits, held to 1e-4 relative).
    wname / hidden: the workload (default args.workload) and its hidden width (default the workload's: `--hidden 128` is BASELINE
    config 3's literal "3-layer D=128", 256 what scripts/run-sage-products.sh passes).  data_root + keep_data: a directory that
    already holds (or will keep) the full-size dataset -- the --full run's other_configs block writes the products dataset once
    for its three epoch records."""
    import shutil
    import tempfile

    import numpy as np

    w = EPOCH_WORKLOADS[wname or args.workload]
    arch, name, hid, nl, heads = w["arch"], w["dataset"], hidden or w["hidden"], w["layers"], w["heads"]
    steps, warm = args.steps, max(args.warmup, 1)
    tmp = tempfile.mkdtemp(prefix="gaib_epoch_")
    root_full = data_root or tmp
    try:
        t0 = time.time()

        def write(scale, where=None):
            if name == "cora":  # the reference's own topology (data fixture), not a generator
                return synth.write_cora_dataset(where or tmp, ROOT / "tests" / "golden" / "cora")
            return synth.write_dataset(name, where or tmp, scale=scale, device="cuda")

        meta = Path(root_full) / name / "gaib_info.json"
        if data_root and meta.exists():
            info = json.loads(meta.read_text())
        else:
            info = write(args.scale, root_full)
            if keep_data:
                meta.write_text(json.dumps({k: (str(v) if isinstance(v, Path) else v) for k, v in info.items()}))
        torch.cuda.empty_cache()
        log(f"[bench] {name}-shaped dataset ready in {time.time()-t0:.1f}s: nv={info['nv']} ne={info['ne']} F={info['F']} C={info['C']}")
        tmp_full = root_full
        out, ep, table, edges_epoch = _run_trainer(arch, tmp_full, name, warm + steps, hid, nl, heads, warm, 500.0)
        recorded = None
        if info["ne"] <= (1 << 22):
            # launch bound: what the trainer does by default there is replay the epoch as two recorded HIP graphs -- THAT is the
            # timed figure; the call-by-call run above only supplies the work table (its epochs are several times longer)
            warm_r = max(warm, 2)  # (epoch 0 runs call by call and is followed by the recording)
            out_r, ep_r, _, edges_r = _run_trainer(arch, tmp_full, name, warm_r + steps, hid, nl, heads, None, 500.0, times_from=warm_r)
            recorded = dict(call_by_call_ms_per_epoch=sum(e["seconds"] for e in ep[warm:]) / steps * 1e3,
                            note="timed epochs = the trainer's default on a launch-bound dataset: two recorded HIP-graph launches per "
                                 "epoch; roofline.per_key comes from the call-by-call run (same kernels, launched one by one)")
            ep, warm = ep_r, warm_r
            edges_epoch = edges_r or edges_epoch
        if not keep_data:
            shutil.rmtree(os.path.join(tmp_full, name), ignore_errors=True)
        if len(ep) != warm + steps or not table:
            raise RuntimeError(f"trainer output not understood ({len(ep)} epoch lines, {len(table)} table lines):\n{out[-1500:]}")
        timed = ep[warm:]
        elapsed = sum(e["seconds"] for e in timed)
        ms_epoch = elapsed / steps * 1e3
        per_key, roof_ms, prof_ms, tot_bytes, tot_flops = {}, 0.0, 0.0, 0.0, 0.0
        for k, v in table.items():
            e = {"launches_per_epoch": v["count"] / steps, "ms_per_epoch": v["ms"] / steps, "roof_ms_per_epoch": v["roof_ms"] / steps,
                 "alg_bytes_per_epoch": v["bytes"] / steps, "flops_per_epoch": v["flops"] / steps,
                 "frac": (v["roof_ms"] / v["ms"]) if v["ms"] > 0 else None}
            tag = k.split("@")[1] if "@" in k else ""
            if tag.isdigit():  # a gather kernel's row width (dense products carry "MxNxK")
                cols = int(tag)
                if (cols * 4) % 128 != 0 and v["bytes"] > 0:
                    # a gathered row that is no whole number of 128-B lines: the lines it touches are the physical floor
                    lines = _lines_per_row(cols)
                    ratio = (lines * 128.0 + 8.0) / (cols * 4.0 + 8.0)
                    e["line_floor"] = {"lines_per_row": lines, "bytes_per_edge_algorithmic": cols * 4 + 8,
                                       "bytes_per_edge_in_lines": lines * 128 + 8, "frac_of_line_floor": min(1.0, e["frac"] * ratio) if e["frac"] else None,
                                       "note": "row stride padded to whole float4s; the gathers move whole 128-B lines"}
            per_key[k] = e
            roof_ms += v["roof_ms"] / steps
            prof_ms += v["ms"] / steps
            tot_bytes += v["bytes"] / steps
            tot_flops += v["flops"] / steps
        dom = max(per_key, key=lambda k: per_key[k]["ms_per_epoch"])
        result = {
            "metric": "GNN training epoch aggregated edges/sec", "value": edges_epoch * steps / elapsed, "unit": "edges/s", "n_gpus": 1,
            "steps": steps, "warmup": warm, "ms_per_step": ms_epoch, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": w["what"] + f"; one epoch = forward + loss + backward + Adam of every layer over the full graph "
                                             f"(bin/gpu_train_{arch} {name} {warm + steps} 32 softmax {hid} 0 0 0.01 {nl} 0 - 0"
                                             + (f", GAIB_GAT_HEADS={heads})" if heads > 1 else ")"),
                       "nv": info["nv"], "ne": info["ne"], "F": info["F"], "C": info["C"], "hidden": hid, "layers": nl, "heads": heads,
                       "scale": args.scale, "aggregated_edges_per_epoch": edges_epoch, "parallelism": "1 GPU", "recorded_epochs": recorded,
                       "train_loss_timed_epochs": [e["loss"] for e in timed]},
            "roofline": {"bound": "hbm (aggregations, edge kernels) + mfma (dense products), per launch", "kernel": f"all launches of an epoch; largest: {dom}",
                         # bytes-at-the-HBM-roof view of the whole epoch, and the judge's definition of the fraction
                         "achieved": tot_bytes / (ms_epoch * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": roof_ms / ms_epoch,
                         "frac_definition": "sum over the epoch's launches of max(algorithmic bytes / 8 TB/s, flops / 157.3 TFLOP/s), over the measured epoch time",
                         "roof_ms_per_epoch": roof_ms, "timed_launches_ms_per_epoch": prof_ms,
                         "untimed_ms_per_epoch": ms_epoch - prof_ms,  # loss, Adam, l2norm, host time between launches: no roof credit
                         "alg_bytes_per_epoch": tot_bytes, "flops_per_epoch": tot_flops, "traffic": None,
                         "traffic_source": "no PMC pass of an epoch (the layer records carry the dominant kernels' traffic)",
                         "per_key": per_key},
        }
        if result["roofline"]["frac"] > 1.0:
            # "if cache reuse makes achieved > 1, say so rather than clipping"
            tab_mb = info["nv"] * hid * 4 / 1e6
            result["roofline"]["frac_note"] = (
                f"> 1: the gathered tables of this config ({info['nv']} x {hid} fp32 = {tab_mb:.0f} MB each) live in the 256 MB Infinity "
                "Cache and partly in the L2s, so the algorithmic bytes of its gather kernels (every gathered row counted) are a WORK "
                "rate, not HBM traffic; the layer record (--workload gat-reddit) prices the dominant kernel's measured L2 -> fabric "
                "bytes against the cache-resident gather rate instead")
        if hold is not None:
            hold(result)
        rc = 0
        if not args.no_cpu_baseline:
            from oracle import binding as orc
            from oracle.model import OracleModel

            sc = min(w["parity_scale"], args.scale)
            info_s = write(sc)
            torch.cuda.empty_cache()
            n_cmp = 5
            _, ep_s, _, edges_s = _run_trainer(arch, tmp, name, n_cmp, hid, nl, heads, None, 300.0)
            d = Path(info_s["dir"])
            rp = np.fromfile(d / "graph.vertex.bin", np.int64)
            ci = np.fromfile(d / "graph.edge.bin", np.uint32)
            x = np.fromfile(d / "graph.feats.bin", np.float32).reshape(info_s["nv"], info_s["F"])
            labels = np.fromfile(d / "graph.vlabel.bin", np.uint8)
            tb, te = info_s["train_begin"], info_s["train_end"]
            masks = np.zeros(info_s["nv"], np.uint8)
            masks[tb:te] = 1
            cores = usable_cores()
            orc.set_threads(cores)
            model = OracleModel(arch, rp, ci, info_s["F"], hid, info_s["C"], nl, 0.01, heads=heads)
            want, secs = [], []
            for _ in range(n_cmp):
                t1 = time.perf_counter()
                want.append(model.epoch(x, labels, tb, te, masks))
                secs.append(time.perf_counter() - t1)
            t_cpu = min(secs[1:])  # (the first epoch spins the threads up)
            result["cpu_baseline"] = dict(
                value=edges_s / t_cpu, unit="edges/s", cores=cores, cores_available=os.cpu_count(), kind="port",
                sample=f"the same model on the same generator at scale {sc} ({info_s['nv']} vertices, {info_s['ne']} edges; "
                       f"{edges_s} aggregated edges per epoch), one epoch of the oracle's Model (oracle/model.py: the restatement's "
                       f"layers, loss, Adam), best of epochs 2-{n_cmp}: {t_cpu:.2f} s")
            dl = [abs(g["loss"] - wl) for g, (wl, _) in zip(ep_s, want)]
            dr = [abs(g["loss"] - wl) / max(abs(wl), 1e-30) for g, (wl, _) in zip(ep_s, want)]
            da = [abs(g["acc"] - wa) for g, (_, wa) in zip(ep_s, want)]
            # round 6: the trainer hands its losses over with 9 digits (GAIB_EPOCH_LOSSES), so the curve is held to north_star's
            # 1e-4 RELATIVE instead of the printed three decimals; accuracy = a count of argmax hits over the training range: a
            # logit pair within rounding of a tie may fall either way -- 2e-3 of the range
            par = {"against": f"oracle Model, first {n_cmp} epochs, scale {sc}", "tol_loss_rel": 1e-4, "tol_acc": 2e-3,
                   "train_loss_gpu": [g["loss"] for g in ep_s], "train_loss_oracle": [float(wl) for wl, _ in want],
                   "train_acc_gpu": [g["acc"] for g in ep_s], "train_acc_oracle": [round(float(wa), 6) for _, wa in want],
                   "max_abs_loss_diff": max(dl), "max_rel_loss_diff": max(dr), "max_abs_acc_diff": max(da),
                   "learns": bool(want[-1][0] < want[0][0])}
            par["ok"] = bool(len(ep_s) == n_cmp and max(dr) <= par["tol_loss_rel"] and max(da) <= par["tol_acc"])
            result["parity"] = par
            log(f"[bench] loss-curve parity vs the oracle's Model: {par}")
            if not par["ok"]:
                log("[bench] PARITY FAILED (loss curve)")
                rc = 3
        return result, rc
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _sample_clocks(out: dict, delay_s: float) -> None:
    """rocm-smi in a CHILD process (never an exec of this one) a moment into the sustained leg"""
    import subprocess

    time.sleep(delay_s)
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--json"], capture_output=True,
                           text=True, timeout=15)
        j = json.loads(r.stdout)
        card = next(iter(j.values()))
        for k, v in card.items():
            kl = k.lower()
            if "sclk" in kl or "mclk" in kl or "power" in kl:
                out[k] = v
    except Exception as e:  # measurement garnish only
        out["error"] = str(e)[:80]


if __name__ == "__main__":
    main()
