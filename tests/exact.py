"""Helpers of the exact tests (tests/test_exact_cpu.py, tests/test_gpu_dense_exact.py, tests/test_gpu_agg_exact.py).

On operands that are small integers every product is an integer and every partial sum, taken in any order, is an integer
below 2^24: fp32 holds each of them exactly, so every correct fp32 kernel -- whatever its tiling, split of K, ring depth or
atomics -- returns the same bits, and the comparison is equality.  A missing or doubled term, a lane that reads its
neighbour's column, a tail summed in lower precision or a stale LDS slot shows at the element where it happens.  The same
holds for values that are integers times one power of two (the regular graph's weights 1/deg and deg^-1/2 * deg^-1/2 at
degrees that are powers of 4).

This module holds what needs no GPU: the generators, which assert the 2^24 bound FROM THE DATA (max(|A| . |B| + |C0|), never
from the shape), the fp64 references with an int64 guard of their own, the placement of an operand at a chosen offset inside a
guarded buffer, the two graphs, and the table of dense cases, which is also the record of the dispatch branches the suite
reaches.  Helpers that touch tensors import torch when called."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import poison as P
from util import csr_from_pairs, random_graph

LIMIT = 1 << 24
NAN_BITS = P.NAN_BITS        # input guards: a read that reaches a sum is visible
OUT_BITS = 0x4B1D5EED        # output guards: a finite pattern (1.03e7) no integer sum of these sizes produces, checked for equality
GUARD = 64


# ---- dense products -----------------------------------------------------------------------------------------------------------------
# form: "nn" C = A . B, "nt" C = A . B^T, "tn" C = A^T . B (gaib_sgemm_ex); "mask" G <- G where mask > 0 else 0, C = A^T . G
# (gaib_sgemm_drelu: A [K x M], G and mask [K x N]).
FORMS = {"nn": (False, False), "nt": (False, True), "tn": (True, False), "mask": (True, False)}


def dense_shapes(form: str, M: int, N: int, K: int):
    tA, tB = FORMS[form]
    return ((K, M) if tA else (M, K)), ((N, K) if tB else (K, N))


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, shape, dtype=np.int16).astype(np.float32)


def assert_bound(absA, absB, absC0, what: str = "") -> float:
    """max(|A| . |B| + |C0|) < 2^24, from the data.  The product of the absolute values is taken in fp32: below the bound every
    partial sum of it is an exact integer, and a sum of non-negative integers that reaches 2^24 in truth reaches it in fp32 too
    (rounding is monotone and 2^24 is a number of the format), so the check cannot pass by its own rounding."""
    top = float((absA @ absB + absC0).max()) if absA.size and absB.size else float(absC0.max())
    assert top < LIMIT, f"{what}: a partial sum may reach {top:.0f} >= 2^24"
    return top


def dense_operands(form: str, M: int, N: int, K: int, seed: int) -> SimpleNamespace:
    """A, B with integers in [-7, 7], C0 with integers in [-4096, 4096], float32 in the layouts ctx.sgemm takes; the masked
    form also a mask with ~10 % exact zeros and ~45 % negatives (49 K + 4096 < 2^24 up to K = 342 000; asserted from the data)"""
    rng = np.random.default_rng([seed, M, N, K, sorted(FORMS).index(form)])
    sa, sb = dense_shapes(form, M, N, K)
    A, B, C0 = _ints(rng, sa, -7, 7), _ints(rng, sb, -7, 7), _ints(rng, (M, N), -4096, 4096)
    mask = None
    if form == "mask":
        u = rng.random(sb, dtype=np.float32)
        mag = _ints(rng, sb, 1, 7)
        mask = np.where(u < 0.10, np.float32(0), np.where(u < 0.55, -mag, mag)).astype(np.float32)
    tA, tB = FORMS[form]
    a, b = np.abs(A), np.abs(B)
    assert_bound(a.T if tA else a, b.T if tB else b, np.abs(C0), f"{form} {M} x {N} x {K}")
    return SimpleNamespace(form=form, M=M, N=N, K=K, A=A, B=B, C0=C0, mask=mask)


def effective_b(ops) -> np.ndarray:
    """B as the product sees it: G0 * (mask > 0) for the masked form"""
    return ops.B if ops.mask is None else np.where(ops.mask > 0, ops.B, np.float32(0)).astype(np.float32)


def check_product(ops, prod) -> None:
    """the guard of the reference: the row sums of prod = op(A) . op(B) equal A . (B . 1) and its column sums (1 . A) . B,
    both taken in int64 numpy on the host -- a wrong fp64 GEMM cannot pass as truth"""
    tA, tB = FORMS[ops.form]
    Ai, Bi = ops.A.astype(np.int64), effective_b(ops).astype(np.int64)
    Ai, Bi = (Ai.T if tA else Ai), (Bi.T if tB else Bi)
    rows, cols = Ai @ Bi.sum(1), Ai.sum(0) @ Bi
    assert np.array_equal(prod.sum(1).cpu().numpy(), rows.astype(np.float64)), "the fp64 reference's row sums are not the int64 ones"
    assert np.array_equal(prod.sum(0).cpu().numpy(), cols.astype(np.float64)), "the fp64 reference's column sums are not the int64 ones"


def dense_ref(ops, accum: bool = False, relu: bool = False, device: str = "cpu"):
    """the fp64 result op(A) . op(B) (+ C0), clamped at 0 for relu, as a float64 tensor on `device` (exact: every partial sum is
    below 2^53).  The product is guarded before it is believed (check_product)."""
    import torch

    tA, tB = FORMS[ops.form]
    key = "_prod_" + device
    if not hasattr(ops, key):
        Bn = effective_b(ops)
        A, B = torch.from_numpy(ops.A).to(device).double(), torch.from_numpy(Bn).to(device).double()
        prod = (A.t() if tA else A) @ (B.t() if tB else B)
        check_product(ops, prod)
        setattr(ops, key, prod)
    ref = getattr(ops, key)
    if accum:
        ref = ref + torch.from_numpy(ops.C0).to(device).double()
    return ref.clamp_min(0) if relu else ref


def placed(t, off: int, guard: int = GUARD, fill: int = NAN_BITS, device=None):
    """a view of t's contents inside a fresh flat buffer [guard | off floats | operand | guard], off in floats (0, 1 or 2 in the
    tests: 0, 4 or 8 bytes past a 16-byte boundary); the operand ends exactly where the trailing guard begins.  Everything
    around the operand holds the bit pattern `fill`: NaN for inputs, OUT_BITS for outputs -- guards_intact checks it afterwards."""
    import torch

    src = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    device = src.device if device is None else device
    n = src.numel()
    buf = torch.empty(2 * guard + off + n, dtype=torch.float32, device=device)
    buf.view(torch.int32).fill_(fill if fill < (1 << 31) else fill - (1 << 32))
    view = buf[guard + off:guard + off + n].view(src.shape)
    view.copy_(src)
    assert view._base is buf and view.data_ptr() - buf.data_ptr() == 4 * (guard + off) and buf.data_ptr() % 16 == 0
    return view


def guards_intact(view, off: int, guard: int = GUARD, fill: int = NAN_BITS) -> bool:
    """the elements before and behind a placed operand still hold `fill`"""
    import torch

    b = view._base.view(torch.int32)
    lo, n = guard + off, view.numel()
    assert b.numel() == 2 * guard + off + n
    return bool((b[:lo] == fill).all()) and bool((b[lo + n:] == fill).all())


# (A, B, C) offsets in floats; the masked form: (A, G, C, mask) -- the mask shares G's offset, then has its own
OFFSETS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 1))
OFFSETS_MASK = tuple(o + (o[1],) for o in OFFSETS) + ((0, 0, 0, 1), (0, 1, 0, 2))

# ---- the dense cases: (branch, form, M, N, K, sgemm_variants) -----------------------------------------------------------------------
# One row per dispatch branch and shape; the comment names the rule in csrc/sgemm.hip / csrc/sgemm_skinny.hip that sends the
# row there (variant 0 = the dispatch's own rule; the work table does not tell the kernels apart, so this table is the record).
# Under a placement that breaks an alignment the rule asks for, the row falls to the next kernel down -- never to an error.
TILED_VARIANTS = (0, 2, 10, 11, 12, 13, 37, 50)   # occupancy 2; 128 x 64, 64 x 128, 64 x 64 tiles; 128 x 128 for NN / NT; 4-byte loads of a row-major A; no split-K
RS = 65537                                        # row-stream M: gaib_sgemm_skinny_try takes M >= 65536
DENSE_CASES = [
    # --- the LDS-tiled kernel (launch<> through dispatch_shape) ---
    ("tiled 64x128", "nn", 33, 65, 129, TILED_VARIANTS),      # dispatch_shape: N > 64 && !AK -> launch<2,2,1,2>; 13 -> <2,2,2,2>; 10 / 11 / 12 the experimental tiles
    ("tiled 64x128", "nt", 33, 65, 129, TILED_VARIANTS),      # the same, B [N][K]
    ("tiled 128x128", "tn", 33, 65, 129, TILED_VARIANTS),     # dispatch_shape: N > 64 && AK -> launch<2,2,2,2>
    ("tiled 256x64", "nt", 257, 33, 31, (0,)),                # dispatch_shape: 32 < N <= 64 -> launch<4,1,2,2>; K < BK: one partial step
    ("tiled 256x32", "nn", 70, 20, 36, (0,)),                 # dispatch_shape: N <= 32 -> launch<4,1,2,1>
    ("tiled split-K", "nn", 300, 130, 516, TILED_VARIANTS),   # launch: tiles < 2 CUs && K >= 512 -> splits (maxs = K / 2 BK); 50: one slab
    ("tiled split-K, K >= 8192", "tn", 65, 130, 9000, (0,)),  # launch: K >= 8192 -> maxs = K / 8 BK
    ("tiled split-K, K < 8192", "tn", 130, 47, 8191, (0,)),   # launch: one below -> maxs = K / 2 BK; odd N on the 256 x 64 tile
    ("tiled, 16-byte loads at 4-byte alignment", "nn", 2708, 16, 1433, (0, 37)),  # gaib_sgemm_ex: av4 = !(A & 3) for a row-major A with K % 4 != 0; 37: 4-byte loads
    ("tiled, one below the register teams", "tn", 128, 128, 32767, (0,)),         # gaib_sgemm_ex: K >= 32768 fails -> dispatch_shape
    # --- the streaming kernel (launch_stream; sgemm_variant 41 forces it wherever stream_shape holds) ---
    ("streaming NT=2", "nn", 31, 47, 128, (41,)),             # launch_stream: 32 < N <= 64 -> GAIB_STREAM(2); M < one row tile
    ("streaming NT=2", "nt", 33, 47, 128, (41,)),             # launch_stream<true>
    ("streaming NT=4, K = 8", "nn", 1, 128, 8, (41,)),        # stream_shape: K >= 8, the smallest; N > 96 -> GAIB_STREAM(4)
    ("streaming, half step", "nn", 65, 47, 12, (41,)),        # stream_shape: K % 4 == 0 with K % 8 == 4
    ("streaming NT=2, ragged", "nt", 999, 33, 252, (41,)),    # 32 < N <= 64, M no multiple of 32
    ("streaming NT=3", "nn", 65, 72, 96, (41,)),              # launch_stream: 64 < N <= 96 -> GAIB_STREAM(3)
    ("streaming NT=1", "nn", 65, 20, 64, (41,)),              # launch_stream: N <= 32 -> GAIB_STREAM(1)
    ("streaming, two slabs", "nt", 3000, 200, 104, (41,)),    # launch_stream: slabs = cdiv(N, 128) = 2
    ("streaming by the automatic rule", "nn", RS, 72, 96, (0,)),  # gaib_sgemm_ex: auto_rule && M >= 65536 && K >= kmin (96)
    # --- the row-stream family (gaib_sgemm_skinny_try, !transA && M >= 65536; 61: family off) ---
    ("row-stream 47 x 64", "nn", RS, 47, 64, (0, 61)),        # ct == 3 && K == 64 -> GAIB_ROWS(4,0,3,1)
    ("row-stream 47 x 128", "nn", RS, 47, 128, (0, 61)),      # ct == 3 && K == 128 -> GAIB_ROWS(8,0,3,1)
    ("row-stream 41 x 256", "nn", 65551, 41, 256, (0, 61)),   # ct == 3 && K == 256 -> GAIB_ROWS(16,0,3,1)
    ("row-stream 128 x 47", "nn", RS, 128, 47, (0, 61)),      # N == 128 && 32 < K <= 48 -> GAIB_ROWS(3,0,8,2)
    ("row-stream 256 x 45", "nn", 65551, 256, 45, (0, 61)),   # N == 256 && 32 < K <= 48 -> GAIB_ROWS(3,0,16,1)
    ("row-stream nt 64 x 41", "nt", RS, 64, 41, (0, 61)),     # transB && N == 64 -> GAIB_ROWS(3,0,4,2,true)
    ("row-stream nt 128 x 47", "nt", RS, 128, 47, (0, 61)),   # transB && N == 128 -> GAIB_ROWS(3,0,8,2,true)
    ("row-stream nt 256 x 48", "nt", 65551, 256, 48, (0, 61)),  # transB && N == 256 -> GAIB_ROWS(3,0,16,1,true)
    ("row-stream 128 x 100", "nn", RS, 128, 100, (0, 61)),    # N == 128 && K == 100 -> GAIB_ROWS(6,1,8,1)
    ("row-stream 256 x 100", "nn", RS, 256, 100, (0, 64, 61)),  # N == 256 && K == 100 -> two slabs of GAIB_ROWS(6,1,8,1); 64: off
    ("row-stream 128 x 128", "nn", 65551, 128, 128, (0, 66, 61)),  # N == 128 && K == 128 -> GAIB_ROWS(8,0,8,1); 66: the streaming kernel
    ("row-stream nt 128 x 128", "nt", RS, 128, 128, (0, 66, 61)),  # the same with transB
    ("row-stream 256 x 256", "nn", RS, 256, 256, (0, 66, 61)),     # N == 256 && K == 256 -> four slabs of GAIB_ROWS(16,0,4,1)
    ("row-stream nt 256 x 256", "nt", 65551, 256, 256, (0, 66, 61)),  # the same with transB
    # --- skinny TN (gaib_sgemm_skinny_try: K >= 65536, M % 4 == 0, 32 < N <= 48; 62: off -> the register teams' narrow form) ---
    ("skinny tn NH=1", "tn", 128, 47, 65537, (0, 62)),        # 64 < M <= 128 -> GAIB_TNS(1,4,2,2)
    ("skinny tn NH=1, smallest", "tn", 68, 33, 65536, (0, 62)),
    ("skinny tn NH=2", "tn", 256, 48, 65540, (0, 62)),        # 192 < M <= 256 -> GAIB_TNS(2,4,2,2); 62: sgemm_tn_reg_kernel<false,2,1,false,2>
    ("skinny tn NH=2, smallest", "tn", 196, 41, 65551, (0, 62)),
    # --- wide TN (gaib_sgemm_wide_tn_try: K >= 65536, N in {128, 256}, 68 <= M <= 112; 67: off -> the register teams) ---
    ("wide tn N=128", "tn", 100, 128, 65537, (0, 67)),        # GAIB_WTN(7,1), plain
    ("wide tn N=256, smallest", "tn", 68, 256, 65536, (0, 67)),  # GAIB_WTN(7,2), plain
    ("wide tn N=256", "tn", 112, 256, 65551, (0, 67)),
    ("wide tn N=128, masked", "mask", 100, 128, 65537, (0, 67)),  # gaib_sgemm_drelu -> GAIB_WTN(7,1) with the mask
    ("wide tn N=256, masked, smallest", "mask", 68, 256, 65536, (0, 67)),
    ("wide tn N=256, masked", "mask", 112, 256, 65551, (0, 67)),
    # --- register teams (launch_tn_reg: transA, M, N <= 256, M % 4 == 0, avec, b_rows_ok, K >= 32768) ---
    ("register 1x1", "tn", 128, 128, 32768, (0, 29, 33)),     # GAIB_TN(1,1); 29: the non-temporal form; 33: contiguous K ranges per team
    ("register 2x2", "tn", 256, 256, 32775, (0, 33)),         # GAIB_TN(2,2)
    ("register 1x2", "tn", 100, 256, 32769, (0,)),            # GAIB_TN(1,2)
    ("register 2x1", "tn", 256, 128, 33000, (0,)),            # GAIB_TN(2,1)
    ("register narrow B, N <= 32, QM=2", "tn", 256, 32, 32768, (0,)),   # narrow && N <= 32 -> sgemm_tn_reg_kernel<false,2,1,false,1>
    ("register narrow B, N <= 32, QM=1", "tn", 12, 7, 32768, (0,)),     # sgemm_tn_reg_kernel<false,1,1,false,1>
    ("register narrow B, N <= 64", "tn", 128, 64, 32769, (0,)),         # narrow -> sgemm_tn_reg_kernel<false,1,1,false,2>
    ("register narrow B, odd N", "tn", 128, 47, 40003, (0, 38)),        # b_rows_ok by N <= 64; 38: the four-tile NUNAL form (N % 4 != 0 && M <= 128)
    ("register odd N above 64, 1x2", "tn", 100, 129, 33000, (0,)),      # b_rows_ok by N % 4 != 0 && M <= 128 && !(B & 3) -> GAIB_TN(1,2) NUNAL
    ("register odd N above 64, 1x1", "tn", 100, 67, 32769, (0,)),       # the same -> GAIB_TN(1,1) NUNAL
    # --- the LDS ring (launch_tn_glds: M > 128 && N > 128 && (mask || 35); 34: the register teams; 28: non-temporal) ---
    ("LDS ring, masked", "mask", 256, 256, 32768, (0, 28, 34)),
    ("LDS ring, masked, ragged", "mask", 132, 252, 40009, (0, 34)),
    ("LDS ring, plain", "tn", 256, 256, 32768, (35,)),
    ("LDS ring, plain, ragged", "tn", 132, 252, 40009, (35,)),
    # --- gaib_sgemm_drelu's own branches ---
    ("register masked 1x1", "mask", 128, 128, 50001, (0, 39, 30, 31)),  # reg_path -> GAIB_TN(1,1) masked, non-temporal; 39: temporal; 30 / 31: launch<2,2,2,2,true,true> with the mask
    ("register masked 1x1, ragged M", "mask", 100, 128, 33000, (0, 39, 30, 31)),
    ("register masked 2x1", "mask", 256, 128, 32768, (0,)),   # GAIB_TN(2,1) masked
    ("register masked 1x2", "mask", 100, 256, 32769, (0,)),   # GAIB_TN(1,2) masked
    ("tiled masked", "mask", 256, 192, 4097, (0,)),           # K < 32768 -> launch<2,2,2,2,true,true>, split-K
    ("two-step, N <= 64", "mask", 16, 64, 500, (0,)),         # !reg_path && N <= 64 -> gaib_d_relu + gaib_sgemm
    ("two-step, M % 4 != 0", "mask", 130, 130, 777, (0,)),    # !aligned -> gaib_d_relu + gaib_sgemm
]


def dense_id(case) -> str:
    branch, form, M, N, K, _ = case
    return f"{form}-{M}x{N}x{K}"


# ---- graphs -------------------------------------------------------------------------------------------------------------------------
CLASSES = (4, 16, 64, 256, 1024)
CLASS_N = {4: 40, 16: 50, 64: 102, 256: 300, 1024: 1046}   # vertices per component: even, above the degree; 1538 in all, no multiple of 16


def _graph(nv, rp, ci, **more) -> SimpleNamespace:
    deg = np.diff(rp)
    rows = np.repeat(np.arange(nv), deg)
    P._ro(rp, ci, deg, rows)
    return SimpleNamespace(nv=nv, ne=len(ci), rp=rp, ci=ci, deg=deg, rows=rows, **more)


@functools.lru_cache(maxsize=None)
def regular_graph(classes=CLASSES, seed: int = 0xC1C, selfloop: bool = False) -> SimpleNamespace:
    """a disjoint union of circulant graphs, one per degree class: every vertex of a component has the class's degree, counting
    the self loop where `selfloop` adds one.  Without self loops component c is C_n(1 .. c/2) (c neighbours); with them it is
    C_n(1 .. c/2 - 1, n/2) plus the loop (c - 1 neighbours and itself).  The vertices are relabelled by a seeded permutation, so
    that row lengths interleave; rows are sorted, duplicate-free, structurally symmetric.  Degrees are powers of 4: deg^-1/2
    and 1/deg are exact powers of two.  `cls[v]` is v's class."""
    rng = np.random.default_rng(seed)
    src, dst, cls, base = [], [], [], 0
    for c in classes:
        n = CLASS_N[c]
        assert n % 2 == 0 and n > c + 1 and c & (c - 1) == 0 and c.bit_length() % 2 == 1  # a power of 4
        v = np.arange(n)
        offs = list(range(1, c // 2 + (0 if selfloop else 1)))
        for o in offs:
            src.append(base + v)
            dst.append(base + (v + o) % n)
        if selfloop:
            src.append(base + v)
            dst.append(base + (v + n // 2) % n)
        cls += [c] * n
        base += n
    nv = base
    perm = rng.permutation(nv)
    src, dst = perm[np.concatenate(src)], perm[np.concatenate(dst)]
    clsv = np.empty(nv, np.int64)
    clsv[perm] = np.array(cls)
    rp, ci = csr_from_pairs(nv, src, dst)
    if selfloop:
        rows = np.repeat(np.arange(nv), np.diff(rp))
        key = np.unique(np.concatenate([rows * nv + ci.astype(np.int64), np.arange(nv) * (nv + 1)]))
        ci = (key % nv).astype(np.uint32)
        rp = np.concatenate([[0], np.cumsum(np.bincount(key // nv, minlength=nv))]).astype(np.int64)
    P._ro(clsv)
    return _graph(nv, rp, ci, cls=clsv, selfloop=selfloop, loop=1 if selfloop else 0)


def check_regular(G) -> None:
    """what regular_graph promises"""
    assert G.nv % 16 != 0 and G.rp[-1] == G.ne
    assert np.array_equal(G.deg, G.cls), "a vertex whose degree is not its class"
    key = G.rows * G.nv + G.ci.astype(np.int64)
    assert np.all(np.diff(key) > 0), "rows not sorted or with duplicates"
    back = np.sort(G.ci.astype(np.int64) * G.nv + G.rows)
    assert np.array_equal(key, back), "not symmetric"
    assert bool((G.rows == G.ci).any()) == G.selfloop and int((G.rows == G.ci).sum()) == (G.nv if G.selfloop else 0)
    assert np.array_equal(G.cls[G.rows], G.cls[G.ci.astype(np.int64)]), "an edge between two classes"
    assert (np.diff(G.cls) != 0).sum() > G.nv // 4, "row lengths do not interleave"


@functools.lru_cache(maxsize=None)
def irregular_graph() -> SimpleNamespace:
    """util.random_graph(3001, 12, power_law=True, hub_deg=1500) with a second hub of 1500 edges at the LAST vertex: with the
    only hub at vertex 0 a mix-up between "index in the heavy list" and "row id" cannot show"""
    nv = 3001
    rp, ci = random_graph(nv, 12, seed=0xE8AC7, power_law=True, hub_deg=1500)
    rows = np.repeat(np.arange(nv), np.diff(rp))
    other = np.random.default_rng(0x2B).choice(np.arange(1, nv - 1), 1500, replace=False)
    rp, ci = csr_from_pairs(nv, np.concatenate([rows, np.full(1500, nv - 1)]), np.concatenate([ci.astype(np.int64), other]))
    G = _graph(nv, rp, ci, hubs=(0, nv - 1), selfloop=False, loop=0)
    assert G.deg[0] > 1024 and G.deg[nv - 1] > 1024 and int((G.deg > 1024).sum()) == 2, "the two hubs are the heavy rows at the default threshold"
    assert (G.deg > 100).sum() > 2 and (G.deg > 8).sum() > 100
    return G


def agg_ref64(G, kind: str, x, ew=None, heads: int = 1) -> np.ndarray:
    """fp64 aggregation from the definition: out[i] = sum over the edges (i, j) of w(i, j) * x[j], per head where the weights
    have heads (poison.weights64 has the five kinds' weights; the sum as a CSR product in fp64, which is exact on these data in
    any order -- test_exact_cpu.py holds it to poison.aggregate64)"""
    from scipy.sparse import csr_matrix

    x = np.asarray(x, np.float64)
    w = P.weights64(G, kind, ew)
    d = x.shape[1]
    if w.ndim == 1:
        w, heads = w[:, None], 1
    dh = d // heads
    out = np.empty((G.nv, d))
    for h in range(heads):
        A = csr_matrix((w[:, h], G.ci.astype(np.int64), G.rp), shape=(G.nv, x.shape[0]))
        out[:, h * dh:(h + 1) * dh] = A @ x[:, h * dh:(h + 1) * dh]
    return out


def agg_operands(G, d: int, d_out: int = 0, heads: int = 1, seed: int = 0, sparse: float = 0.0, kinds=("edge", "edge_t"),
                 unit: float = 1.0) -> SimpleNamespace:
    """x (integers in [-3, 3], [nv x d]; sparse: that share of its entries zeroed, every fifth row
    left dense, for the packed tables), edge weights per head
    in {1, 2, 3} ([ne] for one head), W and W_self ([d x d_out], integers in [-3, 3]), y0 ([nv x d_out]) and agg0 ([nv x d]) with
    integers in [-8, 8].  Asserted from the data: the largest sum of absolute values any output of any weight kind can hold,
    self term and initial value included, is below 2^24 (at degree 1501 and d = 256: 256 * 3 * (9 * 1501 + 3) = 10.4 M).
    kinds: the weight kinds the bound is taken over; without "edge" / "edge_t" among them no edge weights are made.  unit: the
    bound is 2^24 units (the regular graph: every weight is a power of two, the smallest 2^-10, so every term and every partial
    sum is an integer number of 2^-10)."""
    rng = np.random.default_rng([seed, d, d_out, heads, G.nv])
    x = _ints(rng, (G.nv, d), -3, 3)
    if sparse:   # every fifth row stays dense: over the packed row's capacity
        x = np.where((rng.random((G.nv, d)) < sparse) & (np.arange(G.nv) % 5 != 0)[:, None], np.float32(0), x).astype(np.float32)
    ew = _ints(rng, (G.ne, heads), 1, 3)
    agg0, y0 = _ints(rng, (G.nv, d), -8, 8), _ints(rng, (G.nv, max(d_out, 1)), -8, 8)
    W, W_self = _ints(rng, (d, max(d_out, 1)), -3, 3), _ints(rng, (d, max(d_out, 1)), -3, 3)
    edge = "edge" in kinds or "edge_t" in kinds
    top = np.abs(agg0).astype(np.float64)
    for kind in kinds:
        top = np.maximum(top, agg_ref64(G, kind, np.abs(x), ew.max(1)) + np.abs(agg0))
    assert top.max() / unit < LIMIT, f"an aggregate may reach {top.max() / unit:.0f} >= 2^24 units"
    if d_out:
        ytop = top @ np.abs(W).astype(np.float64) + np.abs(x).astype(np.float64) @ np.abs(W_self) + np.abs(y0)
        assert ytop.max() / unit < LIMIT, f"a product may reach {ytop.max() / unit:.0f} >= 2^24 units"
    if heads == 1:
        ew = ew[:, 0].copy()
    return SimpleNamespace(x=x, ew=ew if edge else None, agg0=agg0, y0=y0, W=W, W_self=W_self, d=d, d_out=d_out, heads=heads,
                           top=float(top.max()), ytop=float(ytop.max()) if d_out else 0.0)


UNIT = 2.0 ** -10   # the smallest weight of the regular graph: 1 / 1024


def assert_dyadic(ref64: np.ndarray, unit: float = UNIT) -> None:
    """a reference on the regular graph: every value is an integer number of `unit`s below 2^24 of them"""
    q = ref64 / unit
    assert np.array_equal(q, np.rint(q)) and np.abs(q).max() < LIMIT


# ---- the aggregation cases (tests/test_gpu_agg_exact.py; tests/test_exact_cpu.py asserts the bounds over the same lists) -------------
THRESHOLDS = (1024, 100, 8)
REGULAR_THRESHOLDS = (1024, 1023, 100, 8)          # a row is heavy with MORE edges than the threshold: 1023 makes the 1024 class heavy
SPMM_DIMS = (16, 47, 64, 128, 300, 768)           # 768 with 8 heads crosses the 512-column slab
SPMM_HEADS = {16: (1, 8), 47: (1,), 64: (1, 8), 128: (1, 8), 300: (1,), 768: (1, 8)}
GEMM_SHAPES = ((128, 128), (64, 32), (100, 128), (47, 128), (128, 47), (256, 256), (200, 96), (130, 40), (101, 40))
SELF_SHAPES = ((128, 128), (256, 128))
BF16_SHAPES = ((128, 128), (64, 48))
ZS_SHAPES = ((128, 128), (256, 128))
REGULAR_DIMS = (47, 64, 128, 256)
REGULAR_KINDS = ("gcn", "mean", "mean_t")
