"""GPU suite, dropout with the mask seed in device memory (gaib_dropout_dev; context option drop_seed_dev / GAIB_DROP_SEED_DEV):
the call against gaib_dropout under the slot's seed, bit for bit; the refusals; the recorded call, which draws the next seed on
every replay; and the trainer, whose recorded epochs under dropout print the log of the epochs enqueued call by call.

Every comparison here is of raw bits: the reference is the library's own by-value call under the same seed."""
import os
import re
import subprocess

import pytest
import torch

from graphaibench_amd import capi
from test_gpu_driver import ROOT, make_dataset  # (imported as a module: its tests are collected there, not here)

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
# one trip of the 16-byte-lane loop covers 2 048 workgroups x 256 threads x 4 elements: a second trip, then a tail of 3
N_TWO_TRIPS = 2048 * 256 * 4 + 1024 + 3
SIZES = [0, 1, 3, 4, 5, 255, 1027, N_TWO_TRIPS]
RATES = [0.0, 0.3, 0.9]
SEEDS = [0x5EED0001, M64]  # the second wraps to 0 on the advance


def slot_of(seed):
    """one 8-byte device slot holding `seed` (uint64 bits in an int64 tensor)"""
    return torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64, device="cuda")


def slot_value(slot):
    return int(slot.cpu()[0].item()) & M64


def special_input(n, seed):
    """standard normal values with -0.0, +inf, -inf and a NaN in the leading elements and again from element 64 on"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n + 8, device="cuda", generator=gen)
    special = torch.tensor([-0.0, float("inf"), float("-inf"), float("nan"), 0.0], device="cuda")
    for base in (0, 64, n - 5):
        k = max(0, min(5, n - base)) if base >= 0 else 0
        if k > 0:
            x[base:base + k] = special[:k]
    return x


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def reference(ctx):
    """gaib_dropout's (masks, out) per (n, rate, seed), each computed once on aligned buffers and kept unchanged"""
    cache = {}

    def get(x, rate, seed):
        key = (x.numel(), rate, seed)
        if key not in cache:
            xa = x.clone()  # (a fresh allocation: aligned)
            m = torch.full((x.numel(),), 7, dtype=torch.uint8, device="cuda")
            o = torch.full((x.numel(),), 7.0, device="cuda")
            if x.numel() > 0:
                ctx.dropout(xa, m, o, rate, seed)
            ctx.sync()
            cache[key] = (m, o)
        return cache[key]

    return get


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("n", SIZES)
def test_bits_equal_the_by_value_call(ctx, reference, n, rate):
    """aligned pointers (16-byte lanes + tail), in / out 4 bytes off and masks 1 byte off (the scalar form), out aliasing in --
    under an ordinary seed and under 2^64 - 1, which wraps: masks and out are gaib_dropout's bits and the slot reads seed + 1"""
    vals = special_input(n, 11 + n % 97)[:n]
    torch.cuda.synchronize()
    for seed in SEEDS:
        want_m, want_o = reference(vals, rate, seed)
        for name, off_io, off_m, alias in [("aligned", 0, 0, False), ("in/out + 4 B", 1, 0, False), ("masks + 1 B", 0, 1, False),
                                           ("all shifted", 1, 1, False), ("out is in", 0, 0, True)]:
            src = torch.full((n + 8,), 7.0, device="cuda")
            src[off_io:off_io + n] = vals
            x = src[off_io:off_io + n]
            dst = src if alias else torch.full((n + 8,), 7.0, device="cuda")
            out = dst[off_io:off_io + n]
            mflat = torch.full((n + 8,), 7, dtype=torch.uint8, device="cuda")
            masks = mflat[off_m:off_m + n]
            assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and mflat.data_ptr() % 4 == 0
            slot = slot_of(seed)
            torch.cuda.synchronize()
            if n == 0:
                ctx.dropout_dev(None, None, None, rate, slot)  # NULL tensors: the slot still advances
            else:
                ctx.dropout_dev(x, masks, out, rate, slot)
            ctx.sync()
            what = (n, rate, hex(seed), name)
            assert slot_value(slot) == (seed + 1) & M64, what
            assert torch.equal(masks, want_m), what
            assert torch.equal(bits(out), bits(want_o)), what
            # nothing outside [0, n) was written, and the input is as it was unless out is in
            assert bool((mflat[:off_m] == 7).all()) and bool((mflat[off_m + n:] == 7).all()), what
            assert bool((dst[:off_io] == 7.0).all()) and bool((dst[off_io + n:] == 7.0).all()), what
            if not alias:
                assert torch.equal(bits(x), bits(vals)), what


def test_refusals_write_nothing(ctx):
    """rate 1.0, a NULL d_seed and a slot 4 bytes off its alignment: an error, masks and out untouched, the slot not advanced"""
    n, seed = 1027, 0x5EED0002
    x = torch.randn(n, device="cuda")

    def attempt(rate, slot_kind):
        masks = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        out = torch.full((n,), 7.0, device="cuda")
        words = torch.tensor([seed & 0xFFFFFFFF, seed >> 32, 0x1234, 0x5678], dtype=torch.int32, device="cuda")
        slot = {"ok": words, "null": None, "off": words[1:]}[slot_kind]
        if slot is not None:
            assert slot.data_ptr() % 8 == (4 if slot_kind == "off" else 0)
        torch.cuda.synchronize()
        ran = True
        try:
            ctx.dropout_dev(x, masks, out, rate, slot, scale=1.0)
        except capi.GaibError:
            ran = False
        ctx.sync()
        untouched = bool((masks == 7).all()) and bool((out == 7.0).all())
        return ran, untouched, words.cpu().tolist()

    same = [seed & 0xFFFFFFFF, seed >> 32, 0x1234, 0x5678]
    assert attempt(0.3, "ok") == (True, False, [(seed + 1) & 0xFFFFFFFF, seed >> 32, 0x1234, 0x5678])  # (accepted, for contrast)
    assert attempt(1.0, "ok") == (False, True, same)
    assert attempt(-0.1, "ok") == (False, True, same)
    assert attempt(0.3, "null") == (False, True, same)
    assert attempt(0.3, "off") == (False, True, same)
    # NULL tensors with n > 0
    slot = slot_of(seed)
    assert ctx.lib.gaib_dropout_dev(ctx.h, n, 1.0, 0.3, slot.data_ptr(), None, None, None) != 0
    ctx.sync()
    assert slot_value(slot) == seed


def test_recorded_call_draws_the_next_seed_per_replay(ctx):
    """the reason the call exists: one recorded gaib_dropout_dev, launched three times, leaves gaib_dropout's bits under
    seed0 + 1, + 2, + 3 (the eager call before the recording drew seed0), and the slot ends at seed0 + 4"""
    n, rate, seed0 = 1027 * 4 + 3, 0.3, M64 - 1  # (wraps inside the replays)
    s = capi.Context(0)
    s.own_stream()
    ex = None
    try:
        x = torch.randn(n, device="cuda")
        masks = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        out = torch.full((n,), 7.0, device="cuda")
        slot = slot_of(seed0)
        torch.cuda.synchronize()

        def by_value(seed):
            m, o = torch.empty_like(masks), torch.empty_like(out)
            ctx.dropout(x, m, o, rate, seed & M64)
            ctx.sync()
            return m, o

        s.dropout_dev(x, masks, out, rate, slot)
        s.sync()
        m, o = by_value(seed0)
        assert torch.equal(masks, m) and torch.equal(bits(out), bits(o)) and slot_value(slot) == (seed0 + 1) & M64
        s.capture_begin()
        s.dropout_dev(x, masks, out, rate, slot)
        ex = s.capture_end()
        s.sync()
        assert slot_value(slot) == (seed0 + 1) & M64  # nothing ran during the recording
        nodes = ex.nodes
        assert 1 <= nodes <= 4, nodes  # the draw and the advance
        drawn = []
        for k in range(3):
            ex.launch()
            s.sync()
            m, o = by_value(seed0 + 1 + k)
            assert torch.equal(masks, m) and torch.equal(bits(out), bits(o)), k
            assert slot_value(slot) == (seed0 + 2 + k) & M64, k
            assert ex.nodes == nodes
            drawn.append(masks.clone())
        assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[1], drawn[2])
        assert slot_value(slot) == (seed0 + 4) & M64
    finally:
        if ex is not None:
            ex.close()
        s.close()


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def run_trainer(root, arch, score_drop, feat_drop, **env):
    clean = {k: v for k, v in os.environ.items() if k not in ("GAIB_DROP_SEED_DEV", "GAIB_EPOCH_GRAPH", "GAIB_GAT_HEADS",
                                                              "GAIB_GAT_FUSED_DROP", "GAIB_EPOCH_LOSSES")}
    cmd = [str(ROOT / "bin" / f"gpu_train_{arch}"), "cora", "14", "2", "softmax", "16", score_drop, feat_drop, "0.01", "2", "0", "5",
           "0"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                          env=dict(clean, DATASET_PATH=root, GAIB_EPOCH_LOSSES="1", **env))


def log_of(r):
    """what a run computed: the log's train_loss / train_acc, val_acc and test accuracy fields and the 9-digit loss lines"""
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exact = re.findall(r"^\[gaib prof\] (epoch_losses|epoch_accs)(( \S+)+)$", r.stdout, re.M)
    return (re.findall(r"train_loss ([0-9.]+) train_acc ([0-9.]+)", r.stdout), re.findall(r"val_acc ([0-9.]+)", r.stdout),
            re.findall(r"Test accuracy: ([0-9.]+)", r.stdout), [(k, v.split()) for k, v, _ in exact])


@pytest.mark.parametrize("arch,score_drop,heads", [("gcn", "0", None), ("sage", "0", None), ("gat", "0.3", None), ("gat", "0.3", "8")])
def test_trainer_records_epochs_under_dropout(tmp_path, arch, score_drop, heads):
    """14 epochs with feat_drop = 0.3 (GAT: score_drop = 0.3 as well): (a) as ever, (b) seeds on the device, call by call, (c)
    seeds on the device, recorded -- one log.  A seed frozen in the recording would repeat epoch 1's masks from epoch 2 on."""
    root, *_ = make_dataset(tmp_path)
    extra = {"GAIB_GAT_HEADS": heads} if heads else {}
    runs = {"a": run_trainer(root, arch, score_drop, "0.3", GAIB_EPOCH_GRAPH="0", **extra),
            "b": run_trainer(root, arch, score_drop, "0.3", GAIB_EPOCH_GRAPH="0", GAIB_DROP_SEED_DEV="1", **extra),
            "c": run_trainer(root, arch, score_drop, "0.3", GAIB_EPOCH_GRAPH="1", GAIB_DROP_SEED_DEV="1", **extra)}
    logs = {k: log_of(r) for k, r in runs.items()}
    for k, r in runs.items():
        assert ("recorded as HIP graphs" in r.stderr) == (k == "c"), (k, r.stderr[-1000:])
        assert r.stderr.count("dropout mask seeds: device") == (0 if k == "a" else 1), (k, r.stderr[-1000:])
    a = logs["a"]
    assert len(a[0]) == 14 and len(a[1]) == 2 and len(a[2]) == 1
    assert [k for k, _ in a[3]] == ["epoch_losses", "epoch_accs"] and all(len(v) == 14 for _, v in a[3])
    assert logs["b"] == a
    assert logs["c"] == a
    losses = [float(v) for v in a[3][0][1]]
    assert sum(losses[-3:]) < sum(losses[:3]), losses  # the loss falls (single epochs jitter under dropout)
    if arch == "gat":
        assert all("GAT attention dropout: staged" in r.stdout for r in runs.values())


def test_one_sweep_dropout_stays_call_by_call_and_bad_switch(tmp_path):
    """attention dropout kept in the one sweep (GAIB_GAT_FUSED_DROP=1) takes its seed by value: not recorded, said so, and the
    run is the run without GAIB_DROP_SEED_DEV; a switch value other than 0 / 1 is refused by name"""
    root, *_ = make_dataset(tmp_path)
    env = dict(GAIB_GAT_HEADS="8", GAIB_GAT_FUSED_DROP="1", GAIB_EPOCH_GRAPH="1")
    plain = run_trainer(root, "gat", "0.3", "0", **env)
    dev = run_trainer(root, "gat", "0.3", "0", GAIB_DROP_SEED_DEV="1", **env)
    assert log_of(dev) == log_of(plain)
    assert len(log_of(dev)[0]) == 14
    for r in (plain, dev):
        assert "GAIB_EPOCH_GRAPH=1 ignored" in r.stderr and "recorded as HIP graphs" not in r.stderr, r.stderr[-1000:]
    assert "one sweep" in dev.stderr.split("GAIB_EPOCH_GRAPH=1 ignored")[1].splitlines()[0]
    assert "dropout mask seeds: device" in dev.stderr and "dropout mask seeds" not in plain.stderr
    bad = run_trainer(root, "gcn", "0", "0.3", GAIB_DROP_SEED_DEV="2")
    assert bad.returncode != 0 and "GAIB_DROP_SEED_DEV=2" in bad.stderr and "expected 0 or 1" in bad.stderr
