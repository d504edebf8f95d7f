// gemm_bf16.hip -- C[M x N] (=|+=) A . op(B) for a bf16 table A (M in the millions) and a small fp32 matrix B, on the bf16
// matrix cores WITHOUT rounding B: an fp32 value is exactly the sum of three bf16 values,
//     w0 = rne_bf16(W),  w1 = rne_bf16(W - w0),  w2 = rne_bf16(W - w0 - w1)        (both subtractions are exact in fp32),
// a bf16 x bf16 product is exact in fp32, so three passes of v_mfma_f32_16x16x32_bf16 over the planes w0, w1, w2 add 3 K exact
// terms into an fp32 accumulator: the only rounding is the accumulation's, the class of error of gaib_sgemm_ex -- at 1/16 of
// the fp32 MFMA's cycles per term and half the streamed bytes.  (|W| below about 2^-100: w1 / w2 underflow bf16's range and the
// low bits of W are lost.)
//
// The streamed operand keeps the shape of sgemm_skinny.hip's row-stream kernel: persistent waves, one buffer descriptor per
// row tile, loop-invariant lane offsets, a ring of NBUF register tiles, straight-line rounds.  A lane's 16-byte load IS the
// 8-element A/B fragment of the MFMA (lane (j = l & 15, q = l >> 4): row j, k = 8 (4 s + q) .. + 7 of k-step s).  The product
// is computed transposed (D^T = op(B)^T . A^T): a lane ends up with four consecutive columns of one output row, one 16-byte
// store per 16 x 16 tile.  Old C and the stores go through a per-tile descriptor too: rows past M and columns past N lie
// outside it (loads return zeros, stores are dropped by the hardware), so the last, partial tile runs the loop's code.
//
// The small operand: a workgroup owns a SLAB of 64 output columns and holds the slab's three planes in LDS as ready-made
// fragments -- [plane][column tile][k-step][lane] x 16 B, 3 x K x 64 x 2 B = 96 KB at K = 256 (the whole 256 x 256 matrix would
// be 384 KB; a CU has 160) -- so a fragment read is one conflict-free ds_read_b128 of 1 KB per wave, used by the wave's two
// row tiles (one read per two MFMAs: half of what the LDS sustains beside four waves of 16-cycle MFMAs).  The slabs of one
// row group are workgroups id, id + 8, id + 16, ... of a one-dimensional grid: ids round-robin over the 8 XCDs, so they sit
// on ONE XCD, walk the same row tiles at the same time, and the second .. fourth reader of a line of A finds it in that XCD's
// L2.  (A correctness-neutral placement: elsewhere the re-reads come from the Infinity Cache.)  Sharing the rows through LDS
// inside one workgroup instead would need all of op(B) near one CU, which is what does not fit.
// The split runs in the kernel's prologue, from op(B) in global memory straight into the LDS image (64 KB of fp32 per
// workgroup out of the L2, ~10 VALU instructions per element): no second kernel, no workspace, nothing that waits for the
// host -- safe inside gaib_capture_begin/end.
#include "common.h"
#include <algorithm>

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf8_t __attribute__((ext_vector_type(8)));

constexpr int GB_CT = 4;                // 16-column tiles of a slab
constexpr int GB_RT = 2;                // 16-row tiles of a step
constexpr int GB_ROWS = 16 * GB_RT;     // rows of a step
constexpr int GB_SLAB = 16 * GB_CT;     // columns of a slab
constexpr int GB_NBUF = 3;              // register tiles of the ring: two in flight while one runs on the matrix cores
constexpr int64_t GB_MAX_LDA = 1 << 22; // a step's rows stay inside one descriptor (32 x lda x 2 B <= 2^28)

struct GemmBf16Args {
  const uint16_t* A;
  const float* B;
  float* C;
  int64_t M, lda;
  int N, K;
  int transB, relu;
  int nrg, slabs;  // row groups (four waves each), column slabs
};

// gaib_cast_f32_bf16's rounding (elementwise.hip) on finite values: nearest, ties to even, on the bit pattern
__device__ __forceinline__ unsigned rne_bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ f4 mfma_bf16(u4_t a, u4_t b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8_t, a), __builtin_bit_cast(bf8_t, b), c, 0, 0, 0);
}

// KS: k-steps of 32 (K <= 32 KS; chunks of 8 past K re-read chunk 0 of the row against zeros in the planes)
// Registers: <8, true> sits at 256 VGPRs + 123 AGPRs with nothing spilled -- the ring of three tiles (192 registers at K = 256)
// is the first thing to shrink if an edit to compute() tips it over (tests/test_abi.py holds every kernel to 16 spilled VGPRs).
template <int KS, bool ACC>
__global__ __launch_bounds__(256, 1) void gemm_bf16_kernel(GemmBf16Args g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gb_planes[];  // [3][GB_CT][KS][64] x 16 B
  constexpr int CT = GB_CT, RT = GB_RT, ROWS = GB_ROWS, NBUF = GB_NBUF;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, q = lane >> 4;
  const int K = g.K, N = g.N;
  // workgroup -> (row group, slab): the slabs of a row group are 8 ids apart (one XCD)
  const int per = 8 * g.slabs;
  const int id = (int)blockIdx.x;
  const int slab = (id % per) >> 3;
  const int rg = (id / per) * 8 + (id & 7);
  if (rg >= g.nrg) return;
  const int n0 = slab * GB_SLAB;

  // ---- prologue: the slab of op(B), split into three bf16 planes, as fragments ----
  for (int u = tid; u < CT * KS * 64; u += 256) {
    const int l = u & 63, s = (u >> 6) % KS, ct = (u >> 6) / KS;
    const int n = n0 + 16 * ct + (l & 15), c = 4 * s + (l >> 4);
    const bool on = n < N && 8 * c < K;  // (K % 8 == 0: a chunk is whole or absent)
    unsigned p[3][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 8 * c + e;
      const int64_t at = on ? (g.transB ? (int64_t)n * K + k : (int64_t)k * N + n) : 0;  // (clamped address + select)
      const float w = on ? g.B[at] : 0.f;
      const unsigned b0 = rne_bf16_bits(w);
      const float r1 = w - __uint_as_float(b0 << 16);
      const unsigned b1 = rne_bf16_bits(r1);
      const float r2 = r1 - __uint_as_float(b1 << 16);
      p[0][e] = b0;
      p[1][e] = b1;
      p[2][e] = rne_bf16_bits(r2);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      u4_t v;
#pragma unroll
      for (int h = 0; h < 4; ++h) v[h] = (p[t][2 * h] & 0xffffu) | (p[t][2 * h + 1] << 16);
      *reinterpret_cast<u4_t*>(gb_planes + (((t * CT + ct) * KS + s) * 64 + l) * 16) = v;
    }
  }
  __syncthreads();

  // ---- the row stream ----
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ntiles = (g.M + ROWS - 1) / ROWS;
  const int64_t W = (int64_t)g.nrg * 4;
  const int64_t wid = (int64_t)rg * 4 + wv;
  const bool relu = g.relu != 0;
  int voff[RT][KS], cvoff[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int c = 8 * (4 * s + q) < K ? 4 * s + q : 0;
      voff[rt][s] = 2 * ((16 * rt + j) * (int)g.lda + 8 * c);
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int n = n0 + 16 * ct + 4 * q;  // (N % 4 == 0: a lane's four columns are all inside or all outside)
      cvoff[rt][ct] = n < N ? 4 * ((16 * rt + j) * N + n) : 0x7ffffff0;  // outside every descriptor: reads 0, store dropped
    }
  }
  const int64_t a_bytes = g.M > 0 ? ((g.M - 1) * g.lda + K) * 2 : 0;  // (the last row ends at its column K)
  const int64_t c_bytes = g.M * (int64_t)N * 4;
  u4_t buf[NBUF][RT][KS];
  auto fetch = [&](int slot, int64_t tile) {
    const int64_t off = tile * ROWS * g.lda * 2;
    const int64_t left = a_bytes - off;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(reinterpret_cast<const char*>(g.A) + off), 0, (int)(left < (1 << 30) ? left : (1 << 30)), 0x00020000);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int s = 0; s < KS; ++s) buf[slot][rt][s] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff[rt][s], 0, 0);
    __builtin_amdgcn_sched_barrier(0);  // every load of the tile is issued before the MFMAs that follow
  };
  auto compute = [&](int slot, int64_t tile) {
    const int64_t off = tile * ROWS * (int64_t)N * 4;
    const int64_t left = c_bytes - off;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(reinterpret_cast<char*>(g.C) + off), 0, (int)(left < (1 << 30) ? left : (1 << 30)), 0x00020000);
    // C +=: the old values are requested behind the next tile's operand loads and used after this tile's MFMAs
    u4_t old[ACC ? RT : 1][ACC ? CT : 1];
    if constexpr (ACC) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) old[rt][ct] = __builtin_amdgcn_raw_buffer_load_b128(rc, cvoff[rt][ct], 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    f4 acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const u4_t w = *reinterpret_cast<const u4_t*>(gb_planes + (((t * CT + ct) * KS + s) * 64 + lane) * 16);
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt][ct] = mfma_bf16(w, buf[slot][rt][s], acc[rt][ct]);
        }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        f4 v = acc[rt][ct];
        u4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if constexpr (ACC) v[e] = __uint_as_float(old[rt][ct][e]) + v[e];
          v[e] = (relu && !(v[e] > 0.f)) ? 0.f : v[e];
          o[e] = __float_as_uint(v[e]);
        }
        __builtin_amdgcn_raw_buffer_store_b128(o, rc, cvoff[rt][ct], 0, 0);
      }
  };
  // this wave's tiles: wid + x W, x = 0 .. nw - 1, in straight-line rounds of NBUF through the ring (sgemm_skinny.hip: an exit
  // test between the steps drains the ring); a request past the wave's last tile takes that tile again, never consumed
  const int64_t nw = wid < ntiles ? (ntiles - wid + W - 1) / W : 0;
  auto tile_of = [&](int64_t x) { return wid + (x < nw ? x : nw - 1) * W; };
  if (nw > 0) {
#pragma unroll
    for (int b = 0; b < NBUF - 1; ++b) fetch(b, tile_of(b));
    int64_t x = 0;
    for (; x + NBUF <= nw; x += NBUF) {
#pragma unroll
      for (int b = 0; b < NBUF; ++b) {
        fetch((b + NBUF - 1) % NBUF, tile_of(x + b + NBUF - 1));
        compute(b, wid + (x + b) * W);
      }
    }
#pragma unroll
    for (int b = 0; b < NBUF - 1; ++b)
      if (x + b < nw) compute(b, wid + (x + b) * W);
  }
}

struct GemmBf16Tag {
  char s[28];
  GemmBf16Tag(int64_t M, int64_t N, int64_t K) { snprintf(s, sizeof(s), "%lldx%lldx%lld", (long long)M, (long long)N, (long long)K); }
};

template <int KS>
int launch_gemm_bf16(gaib_ctx* ctx, const GemmBf16Args& a, int accum) {
  const size_t lds = (size_t)3 * GB_CT * KS * 1024;
  const unsigned blocks = (unsigned)(((a.nrg + 7) / 8) * 8 * a.slabs);
  // (the attribute is set per launch, as everywhere in this library: it belongs to the function ON the current device, and a
  // process may hold contexts on several devices)
  if (accum) {
    GAIB_HIP(hipFuncSetAttribute((const void*)gemm_bf16_kernel<KS, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    gemm_bf16_kernel<KS, true><<<blocks, 256, lds, ctx->stream>>>(a);
  } else {
    GAIB_HIP(hipFuncSetAttribute((const void*)gemm_bf16_kernel<KS, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    gemm_bf16_kernel<KS, false><<<blocks, 256, lds, ctx->stream>>>(a);
  }
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

bool gemm_bf16_shape_ok(const gaib_ctx* ctx, int N, int K, int64_t lda) {
  return ctx->gemm_bf16_kernel != 0 && K >= 8 && K <= 256 && K % 8 == 0 && N >= 4 && N <= 256 && N % 4 == 0 && lda >= K &&
         lda % 8 == 0 && lda <= GB_MAX_LDA;
}

}  // namespace

extern "C" int gaib_gemm_bf16_cover(gaib_ctx* ctx, int transB, int N, int K, int64_t lda) {
  (void)transB;  // both forms are covered alike
  return ctx && gemm_bf16_shape_ok(ctx, N, K, lda) ? 1 : 0;
}

extern "C" int gaib_gemm_bf16(gaib_ctx* ctx, int transB, int64_t M, int N, int K, int64_t lda, const uint16_t* d_A_bf16,
                              const float* d_B, int flags, float* d_C) {
  GAIB_CHECK(ctx, "gaib_gemm_bf16: NULL ctx");
  GAIB_CHECK(M >= 0, "gaib_gemm_bf16: M < 0");
  GAIB_CHECK((flags & ~(GAIB_ACCUMULATE | GAIB_RELU)) == 0, "gaib_gemm_bf16: unknown flag in %d", flags);
  if (!gemm_bf16_shape_ok(ctx, N, K, lda) || (((uintptr_t)d_A_bf16 | (uintptr_t)d_C) & 15) != 0 || ((uintptr_t)d_B & 3) != 0) {
    gaib_set_error("gaib_gemm_bf16: not covered (8 <= K <= 256, K %% 8 == 0; 4 <= N <= 256, N %% 4 == 0; lda >= K, lda %% 8 == 0, "
                   "lda <= %lld; table and C on 16-byte boundaries; option gemm_bf16_kernel = 1): N %d, K %d, lda %lld -- use gaib_sgemm_ex",
                   (long long)GB_MAX_LDA, N, K, (long long)lda);
    return GAIB_ERR_UNSUPPORTED;
  }
  if (M == 0) return GAIB_OK;
  GAIB_CHECK(d_A_bf16 && d_B && d_C, "gaib_gemm_bf16: NULL argument");
  GAIB_CHECK((const void*)d_A_bf16 != (const void*)d_C && (const void*)d_B != (const void*)d_C, "gaib_gemm_bf16: C must not alias an operand");
  GemmBf16Args a;
  a.A = d_A_bf16;
  a.B = d_B;
  a.C = d_C;
  a.M = M;
  a.lda = lda;
  a.N = N;
  a.K = K;
  a.transB = transB ? 1 : 0;
  a.relu = (flags & GAIB_RELU) ? 1 : 0;
  a.slabs = (N + GB_SLAB - 1) / GB_SLAB;
  // one workgroup (four waves, one per SIMD) per CU; the row groups share the CUs with their slabs
  const int64_t ntiles = cdiv64(M, GB_ROWS);
  const int by_cus = std::max(8, ctx->num_cus / a.slabs / 8 * 8);
  a.nrg = (int)std::min<int64_t>(by_cus, cdiv64(ntiles, 4));
  const int accum = (flags & GAIB_ACCUMULATE) ? 1 : 0;
  const double bytes = 2.0 * (double)M * K + 4.0 * (double)M * N * (accum ? 2.0 : 1.0) + 4.0 * (double)K * N;
  const double flops = 2.0 * (double)M * (double)N * (double)K;
  GAIB_HIP(hipSetDevice(ctx->device));
  ProfScope ps(ctx, "gemm_bf16", bytes, flops, 0, GemmBf16Tag(M, N, K).s);
  if (K <= 32) return launch_gemm_bf16<1>(ctx, a, accum);
  if (K <= 64) return launch_gemm_bf16<2>(ctx, a, accum);
  if (K <= 128) return launch_gemm_bf16<4>(ctx, a, accum);
  return launch_gemm_bf16<8>(ctx, a, accum);
}
