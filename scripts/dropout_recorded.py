"""Recorded epochs under dropout (option drop_seed_dev / GAIB_DROP_SEED_DEV=1) against the same epochs enqueued
call by call, and gaib_dropout_dev against gaib_dropout.

Dataset: the cora topology of tests/golden with seeded synthetic features (make_dataset of tests/test_gpu_driver.py).  Every leg
runs with the option on.  Trainer legs, each one process of bin/gpu_train_* under its own `timeout`, GAIB_EPOCH_TIMES=5 (the
epochs' train_time at full precision from epoch 5 on), interleaved: round i runs every leg once, so drift of the box hits all of
them alike; a leg's figure for a round is the median of that process's epochs, and the record holds median (min - max) over the
rounds, in ms:
  gcn   2-layer GCN, hidden 16, feat_drop 0.5                                   GAIB_EPOCH_GRAPH=0 against 1
  gat   2-layer GAT, GAIB_GAT_HEADS=8, hidden 64, feat_drop = score_drop = 0.6  GAIB_EPOCH_GRAPH=0 against 1
Kernel legs, one child process, interleaved per iteration between event pairs, median (min - max) in ms:
  gaib_dropout against gaib_dropout_dev at 2 449 029 x 128 elements, rate 0.5
A leg that fails or runs into its time limit ends the run: nothing further is started.

    python scripts/dropout_recorded.py OUT.json [--rounds 5] [--epochs 100] [--iters 20] [--timeout 300]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
sys.path.insert(0, str(ROOT / "tests"))

ROWS, COLS, RATE = 2449029, 128, 0.5
TRAINER_LEGS = {
    # name: (binary, hidden, score_drop, feat_drop, extra environment)
    "gcn": ("gpu_train_gcn", "16", "0", "0.5", {}),
    "gat": ("gpu_train_gat", "64", "0.6", "0.6", {"GAIB_GAT_HEADS": "8"}),
}


def summarise(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), n=len(ms))


def kernel_child(iters, out_path):
    import torch

    from bf16_gat import time_legs
    from graphaibench_amd import capi

    ctx = capi.Context(0)
    n = ROWS * COLS
    x = torch.randn(n, device="cuda")
    out = torch.empty(n, device="cuda")
    masks = torch.empty(n, dtype=torch.uint8, device="cuda")
    slot = torch.tensor([0x5EED], dtype=torch.int64, device="cuda")
    seed = [0x5EED]

    def by_value():
        ctx.dropout(x, masks, out, RATE, seed[0])
        seed[0] += 1

    def seed_on_device():
        ctx.dropout_dev(x, masks, out, RATE, slot)

    r = dict(elements=n, rate=RATE, iters=iters, bytes_per_call=9 * n, stream_copy_gbs_before=ctx.probe_stream_copy())
    r["ms"] = time_legs({"gaib_dropout": by_value, "gaib_dropout_dev": seed_on_device}, iters)
    r["stream_copy_gbs_after"] = ctx.probe_stream_copy()
    ctx.close()
    Path(out_path).write_text(json.dumps(r) + "\n")


def trainer_run(root, leg, recorded, epochs, limit):
    """one process: its epochs' train_time in ms (from epoch 5 on), or the exit status where it failed"""
    exe, hidden, score_drop, feat_drop, extra = TRAINER_LEGS[leg]
    cmd = ["timeout", "-k", "10", str(limit), str(ROOT / "bin" / exe), "cora", str(epochs), "2", "softmax", hidden, score_drop,
           feat_drop, "0.01", "2", "0", "1000", "0"]
    env = dict(os.environ, DATASET_PATH=root, GAIB_DROP_SEED_DEV="1", GAIB_EPOCH_GRAPH="1" if recorded else "0",
               GAIB_EPOCH_TIMES="5", **extra)
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if p.returncode != 0:
        return p.returncode, p.stderr[-500:]
    if ("recorded as HIP graphs" in p.stderr) != recorded or "dropout mask seeds: device" not in p.stderr:
        return -1, "the run did not take the asked path: " + p.stderr[-500:]
    secs = re.search(r"^\[gaib prof\] epoch_seconds(( \S+)+)$", p.stdout, re.M).group(1).split()
    return 0, [1e3 * float(s) for s in secs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per process")
    ap.add_argument("--kernel-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernel_child:
        kernel_child(args.iters, args.kernel_child)
        return
    from test_gpu_driver import make_dataset

    rec = dict(what="epochs under dropout with the mask seeds in device memory (drop_seed_dev = 1): recorded as HIP graphs against "
                    "call by call; gaib_dropout_dev against gaib_dropout; measured once",
               dataset="cora topology, 96 synthetic feature columns", rounds=args.rounds, epochs_per_process=args.epochs,
               timed_from_epoch=5, trainer={}, kernel=None)
    names = [(leg, mode) for leg in TRAINER_LEGS for mode in ("call_by_call", "recorded")]
    per_round = {f"{leg}_{mode}": [] for leg, mode in names}
    with tempfile.TemporaryDirectory() as tmp:
        root = make_dataset(Path(tmp))[0]
        for _ in range(args.rounds):
            for leg, mode in names:
                rc, got = trainer_run(root, leg, mode == "recorded", args.epochs, args.timeout)
                if rc != 0:  # a fault, an abort or the time limit: nothing more is started on the device
                    rec["stopped"] = dict(leg=f"{leg}_{mode}", exit_status=rc, stderr=got)
                    break
                per_round[f"{leg}_{mode}"].append(statistics.median(got))
            if "stopped" in rec:
                break
        for k, v in per_round.items():
            if v:
                rec["trainer"][k] = dict(epoch_ms=summarise(v), per_round_medians_ms=v)
        if "stopped" not in rec:
            part = Path(tmp) / "kernel.json"
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, str(Path(__file__).resolve()), args.out, "--kernel-child",
                   str(part), "--iters", str(args.iters)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                rec["stopped"] = dict(leg="kernel", exit_status=rc)
            else:
                rec["kernel"] = json.loads(part.read_text())
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec, indent=1))
    sys.exit(1 if "stopped" in rec else 0)


if __name__ == "__main__":
    main()
