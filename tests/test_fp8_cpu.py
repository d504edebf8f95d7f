"""CPU suite, fp8 feature tables with per-row scales: the row stride rule through the built library, and
a restatement of the scale rule and of the cast -- the reference the GPU suite (tests/test_gpu_fp8.py) holds the device cast
to -- checked against hand-computed rows."""
import ctypes

import numpy as np
import torch

from graphaibench_amd import capi

FP8_MAX = 448.0


def row_exponents(x):
    """k per row of x (float32 [rows x len]): the smallest integer with amax * 2^-k <= 448, amax over the row's finite
    elements, clamped to [-126, 120]; 0 for a row with no non-zero finite element"""
    x = np.asarray(x, np.float32)
    a = np.where(np.isfinite(x), np.abs(x), np.float32(0)).astype(np.float32)
    amax = a.max(axis=1) if x.shape[1] else np.zeros(x.shape[0], np.float32)
    m, e = np.frexp(amax.astype(np.float64))  # amax = m * 2^e, m in [0.5, 1); 448 = 0.875 * 2^9
    k = e - 9 + (m > 0.875)
    k = np.clip(k, -126, 120)
    return np.where(amax == 0, 0, k).astype(np.int64)


def cast_rows(x, ld):
    """(q uint8 [rows x ld], scale float32 [rows], k): x * 2^-k in fp32, then torch's CPU conversion to float8_e4m3fn
    (round to nearest even); the pad bytes are 0.  Non-finite inputs: whatever torch gives -- the contract there is the class
    and the sign, which the callers check separately."""
    x = np.ascontiguousarray(x, np.float32)
    rows, ln = x.shape
    k = row_exponents(x)
    inv = np.ldexp(np.float32(1), -k).astype(np.float32)
    s = (x * inv[:, None]).astype(np.float32)
    q = np.zeros((rows, ld), np.uint8)
    q[:, :ln] = torch.from_numpy(s).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return q, np.ldexp(np.float32(1), k).astype(np.float32), k


def widen_rows(q, scale, ln):
    """float32 [rows x ln]: f32(q) * scale, both steps exact"""
    f = torch.from_numpy(np.ascontiguousarray(q[:, :ln])).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    return (f * np.asarray(scale, np.float32)[:, None]).astype(np.float32)


def test_row_stride_rule():
    lib = capi.load()
    for ln, want in [(1, 4), (3, 4), (47, 64), (64, 64), (100, 128), (128, 128), (129, 256), (256, 256), (300, 384),
                     (4, 4), (5, 8), (0, 0), (384, 384), (1000, 1024)]:
        ld = ctypes.c_int64(-1)
        assert lib.gaib_fp8_row_stride(ln, ctypes.byref(ld)) == 0
        assert ld.value == want, (ln, ld.value, want)
    assert lib.gaib_fp8_row_stride(-1, ctypes.byref(ld)) != 0
    assert lib.gaib_fp8_row_stride(8, None) != 0


def test_scale_rule_on_hand_computed_rows():
    rows = np.zeros((7, 5), np.float32)
    rows[0] = [448.0, -3.0, 0.5, 0.0, 1.0]
    rows[1] = [1.0, -449.0, 0.5, 0.0, 1.0]
    rows[2] = [1.0, -1.0, 0.5, 0.0, 0.25]
    rows[3] = [1.75 * 2.0 ** -8, 2.0 ** -20, 0.0, 0.0, 0.0]
    rows[4] = 0.0
    rows[5] = [2.0 ** -140, 0.0, -(2.0 ** -149), 0.0, 0.0]
    rows[6] = [np.inf, np.nan, -np.inf, 3.0, -0.0]  # amax over the finite elements: 3 = 0.75 * 2^2 -> k = -7
    k = row_exponents(rows)
    assert k.tolist() == [0, 1, -8, -16, 0, -126, -7], k.tolist()
    # the definition itself: amax * 2^-k <= 448 < amax * 2^-(k - 1), away from the clamps
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((4000, 9)) * np.exp2(rng.integers(-60, 60, (4000, 1)))).astype(np.float32)
    k = row_exponents(x)
    amax = np.abs(x).max(axis=1).astype(np.float64)
    assert np.all(np.ldexp(amax, -k) <= FP8_MAX) and np.all(np.ldexp(amax, -(k - 1)) > FP8_MAX)
    # the largest floats need no upper clamp; the smallest sit on the lower one
    big = np.array([[np.finfo(np.float32).max], [2.0 ** 127]], np.float32)
    assert row_exponents(big).tolist() == [120, 119]


def test_cast_restatement_on_hand_computed_rows():
    x = np.array([[448.0, 1.0, -0.0625, 0.0], [1.0, 0.5, 2.0 ** -17, -(2.0 ** -18)], [0.0, 0.0, 0.0, 0.0]], np.float32)
    q, scale, k = cast_rows(x, 8)
    assert k.tolist() == [0, -8, 0] and scale.tolist() == [1.0, 2.0 ** -8, 1.0]
    # row 0: 448 = 0x7e, 1.0 = 0x38, -2^-4 = 0x80 | 0x18; row 1: 256 = 0x78, 128 = 0x70, 2^-9 = the smallest subnormal 0x01,
    # -2^-10 = a tie between 0 and it: to even, -0
    assert q[0].tolist() == [0x7e, 0x38, 0x98, 0, 0, 0, 0, 0]
    assert q[1].tolist() == [0x78, 0x70, 0x01, 0x80, 0, 0, 0, 0]
    assert not q[2].any()
    w = widen_rows(q, scale, 4)
    assert w[0].tolist() == [448.0, 1.0, -0.0625, 0.0] and w[1].tolist() == [1.0, 0.5, 2.0 ** -17, -0.0]
