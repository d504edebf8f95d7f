// sgemm_split.hip -- C[M x N] (=|+=) A . op(B) for fp32 A (M in the millions) and a small fp32 matrix B, on the bf16 matrix
// cores with BOTH operands split exactly: an fp32 value is the sum of three bf16 values, a bf16 x bf16 product is exact in
// fp32, so the nine plane products a_p . b_q (p, q = 0 .. 2) of every term enter an fp32 accumulator of
// v_mfma_f32_16x16x32_bf16 and the only rounding is the accumulation's -- at 9/16 of the fp32 MFMA's cycles per term.
//
// gemm_bf16.hip is the map; what is kept from it: persistent waves, one workgroup per CU; a SLAB of 64 output columns whose
// three planes of op(B) (rne_bf16 of the value and of its two residuals: that kernel's rule, that kernel's bits) live in LDS as
// ready-made fragments [plane][column tile][k-step][lane] x 16 B (96 KB at K = 256), written by the kernel's prologue; the
// slabs of a row group 8 workgroup ids apart (one XCD); the transposed product (a lane ends with four consecutive columns of
// one output row: one 16-byte store per 16 x 16 tile); per-tile buffer descriptors for A, old C and the stores; the
// straight-line ring with its drain.
//
// What changes is the streamed side.  Lane (j = l & 15, q = l >> 4) holds row j, k = 8 (4 s + q) .. + 7 of k-step s as TWO
// 16-byte fp32 loads (8 registers), so a step is ONE 16-row tile and the ring of three tiles is 3 x KS x 8 registers (192 at
// K = 256).  A half of 4 columns at or past K is requested outside the descriptor and arrives as zeros in the registers: the
// columns K .. lda - 1 of a row (and the rows past M, outside the descriptor too) are never consumed.
// The split of a k-step's 8 values runs in registers just before its MFMAs, by TRUNCATION:
//     t0 = a & 0xffff0000,  r1 = a - t0,  t1 = r1 & 0xffff0000,  r2 = r1 - t1        (both subtractions exact: r1 has at most 16
// significant bits, r2 at most 8, so r2 IS a bf16 value), planes = the high halves of a, r1, r2, packed in pairs with one
// v_perm_b32 each: 5.5 VALU instructions per element, 44 per k-step beside its 36 MFMAs (4 column tiles x 3 planes of B x
// 3 planes of A; a B fragment read from LDS feeds three MFMAs).  Truncation cannot overflow: FLT_MAX splits into finite planes.
// |a| below about 2^-100: r2 leaves bf16's normal range and low bits may be lost.  A non-finite a: inf - inf = NaN in r1, so
// the row's outputs become NaN (an infinity surfaces as NaN), and only that row's: a lane's MFMA B-operand is one row.
// The split of k-step s + 1 is placed between the MFMA groups of k-step s, for the scheduler to hide under the matrix cores.
//
// Every output element is produced by one wave in one fixed instruction sequence (k-steps ascending; per k-step the planes of
// B ascending, per plane of B the planes of A ascending): bit-identical from run to run and however M is spread over waves.
#include "split_planes.h"
#include <algorithm>

namespace {

constexpr int SS_CT = 4;                // 16-column tiles of a slab
constexpr int SS_ROWS = 16;             // rows of a step: one row tile
constexpr int SS_SLAB = 16 * SS_CT;     // columns of a slab
constexpr int SS_NBUF = 3;              // register tiles of the ring: two in flight while one runs on the matrix cores
constexpr int64_t SS_MAX_LDA = 1 << 22; // a tile's rows stay inside one descriptor (16 x lda x 4 B <= 2^28)

struct SgemmSplitArgs {
  const float* A;
  const float* B;
  float* C;
  int64_t M, lda;
  int N, K;
  int transB, relu;
  int nrg, slabs;  // row groups (four waves each), column slabs
};

// gaib_cast_f32_bf16's rounding (elementwise.hip) on finite values, as in gemm_bf16.hip: nearest, ties to even
__device__ __forceinline__ unsigned ss_rne_bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// KS: k-steps of 32 (K <= 32 KS)
template <int KS, bool ACC>
__global__ __launch_bounds__(256, 1) void sgemm_split_kernel(SgemmSplitArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ss_planes[];  // [3][SS_CT][KS][64] x 16 B
  constexpr int CT = SS_CT, ROWS = SS_ROWS, NBUF = SS_NBUF;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, q = lane >> 4;
  const int K = g.K, N = g.N;
  // workgroup -> (row group, slab): the slabs of a row group are 8 ids apart (one XCD)
  const int per = 8 * g.slabs;
  const int id = (int)blockIdx.x;
  const int slab = (id % per) >> 3;
  const int rg = (id / per) * 8 + (id & 7);
  if (rg >= g.nrg) return;
  const int n0 = slab * SS_SLAB;

  // ---- prologue: the slab of op(B), split into gemm_bf16.hip's three bf16 planes, as fragments ----
  for (int u = tid; u < CT * KS * 64; u += 256) {
    const int l = u & 63, s = (u >> 6) % KS, ct = (u >> 6) / KS;
    const int n = n0 + 16 * ct + (l & 15), c = 4 * s + (l >> 4);
    unsigned p[3][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 8 * c + e;
      const bool on = n < N && k < K;  // (K % 4 == 0: a chunk of 8 may be half inside)
      const int64_t at = on ? (g.transB ? (int64_t)n * K + k : (int64_t)k * N + n) : 0;  // (clamped address + select)
      const float w = on ? g.B[at] : 0.f;
      const unsigned b0 = ss_rne_bf16_bits(w);
      const float r1 = w - __uint_as_float(b0 << 16);
      const unsigned b1 = ss_rne_bf16_bits(r1);
      const float r2 = r1 - __uint_as_float(b1 << 16);
      p[0][e] = b0;
      p[1][e] = b1;
      p[2][e] = ss_rne_bf16_bits(r2);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      u4_t v;
#pragma unroll
      for (int h = 0; h < 4; ++h) v[h] = (p[t][2 * h] & 0xffffu) | (p[t][2 * h + 1] << 16);
      *reinterpret_cast<u4_t*>(ss_planes + (((t * CT + ct) * KS + s) * 64 + l) * 16) = v;
    }
  }
  __syncthreads();

  // ---- the row stream ----
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ntiles = (g.M + ROWS - 1) / ROWS;
  const int64_t W = (int64_t)g.nrg * 4;
  const int64_t wid = (int64_t)rg * 4 + wv;
  const bool relu = g.relu != 0;
  int voff[KS][2], cvoff[CT];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = 8 * (4 * s + q) + 4 * h;  // (K % 4 == 0: a half of 4 columns is all inside or all outside)
      voff[s][h] = k < K ? 4 * (j * (int)g.lda + k) : SS_OUTSIDE;
    }
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int n = n0 + 16 * ct + 4 * q;  // (N % 4 == 0: a lane's four columns are all inside or all outside)
    cvoff[ct] = n < N ? 4 * (j * N + n) : SS_OUTSIDE;
  }
  const int64_t a_bytes = g.M > 0 ? ((g.M - 1) * g.lda + K) * 4 : 0;  // (the last row ends at its column K)
  const int64_t c_bytes = g.M * (int64_t)N * 4;
  u4_t buf[NBUF][KS][2];
  auto fetch = [&](int slot, int64_t tile) {
    const int64_t off = tile * ROWS * g.lda * 4;
    const int64_t left = a_bytes - off;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(reinterpret_cast<const char*>(g.A) + off), 0, (int)(left < (1 << 30) ? left : (1 << 30)), 0x00020000);
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int h = 0; h < 2; ++h) buf[slot][s][h] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff[s][h], 0, 0);
    __builtin_amdgcn_sched_barrier(0);  // every load of the tile is issued before the MFMAs that follow
  };
  auto compute = [&](int slot, int64_t tile) {
    const int64_t off = tile * ROWS * (int64_t)N * 4;
    const int64_t left = c_bytes - off;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(reinterpret_cast<char*>(g.C) + off), 0, (int)(left < (1 << 30) ? left : (1 << 30)), 0x00020000);
    // C +=: the old values are requested behind the next tile's operand loads and used after this tile's MFMAs
    u4_t old[ACC ? CT : 1];
    if constexpr (ACC) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) old[ct] = __builtin_amdgcn_raw_buffer_load_b128(rc, cvoff[ct], 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    f4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f4{0.f, 0.f, 0.f, 0.f};
    u4_t pl[2][3];  // the planes of this k-step and of the next
    ss_split8(buf[slot][0][0], buf[slot][0][1], pl[0]);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int tb = 0; tb < 3; ++tb) {
        u4_t w[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          w[ct] = *reinterpret_cast<const u4_t*>(ss_planes + (((tb * CT + ct) * KS + s) * 64 + lane) * 16);
#pragma unroll
        for (int ta = 0; ta < 3; ++ta)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) acc[ct] = ss_mfma(w[ct], pl[s & 1][ta], acc[ct]);
        if (tb == 0 && s + 1 < KS) ss_split8(buf[slot][s + 1][0], buf[slot][s + 1][1], pl[(s + 1) & 1]);
      }
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      f4 v = acc[ct];
      u4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (ACC) v[e] = __uint_as_float(old[ct][e]) + v[e];
        v[e] = (relu && !(v[e] > 0.f)) ? 0.f : v[e];
        o[e] = __float_as_uint(v[e]);
      }
      __builtin_amdgcn_raw_buffer_store_b128(o, rc, cvoff[ct], 0, 0);
    }
  };
  // this wave's tiles: wid + x W, x = 0 .. nw - 1, in straight-line rounds of NBUF through the ring (gemm_bf16.hip: an exit
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

struct SgemmSplitTag {
  char s[28];
  SgemmSplitTag(int64_t M, int64_t N, int64_t K) { snprintf(s, sizeof(s), "%lldx%lldx%lld", (long long)M, (long long)N, (long long)K); }
};

template <int KS>
int launch_sgemm_split(gaib_ctx* ctx, const SgemmSplitArgs& a, int accum) {
  const size_t lds = (size_t)3 * SS_CT * KS * 1024;
  const unsigned blocks = (unsigned)(((a.nrg + 7) / 8) * 8 * a.slabs);
  // (the attribute is set per launch, as everywhere in this library: it belongs to the function ON the current device)
  if (accum) {
    GAIB_HIP(hipFuncSetAttribute((const void*)sgemm_split_kernel<KS, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    sgemm_split_kernel<KS, true><<<blocks, 256, lds, ctx->stream>>>(a);
  } else {
    GAIB_HIP(hipFuncSetAttribute((const void*)sgemm_split_kernel<KS, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    sgemm_split_kernel<KS, false><<<blocks, 256, lds, ctx->stream>>>(a);
  }
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

bool sgemm_split_shape_ok(const gaib_ctx* ctx, int N, int K, int64_t lda) {
  return ctx->sgemm_split_kernel != 0 && K >= 4 && K <= 256 && K % 4 == 0 && N >= 4 && N <= 256 && N % 4 == 0 && lda >= K &&
         lda % 4 == 0 && lda <= SS_MAX_LDA;
}

}  // namespace

// the launcher's grid rule: column slabs and row groups (four waves each; wave w of W = 4 nrg takes the 16-row tiles
// w, w + W, w + 2 W, ...) -- one workgroup (one wave per SIMD) per CU, the row groups share the CUs with their slabs
static void sgemm_split_grid(const gaib_ctx* ctx, int64_t M, int N, int* slabs, int* nrg) {
  *slabs = (N + SS_SLAB - 1) / SS_SLAB;
  const int by_cus = std::max(8, ctx->num_cus / *slabs / 8 * 8);
  *nrg = (int)std::min<int64_t>(by_cus, cdiv64(cdiv64(M, SS_ROWS), 4));
}

extern "C" int gaib_sgemm_split_cover(gaib_ctx* ctx, int transB, int N, int K, int64_t lda) {
  (void)transB;  // both forms are covered alike
  return ctx && sgemm_split_shape_ok(ctx, N, K, lda) ? 1 : 0;
}

extern "C" int gaib_sgemm_split(gaib_ctx* ctx, int transB, int64_t M, int N, int K, int64_t lda, const float* d_A,
                                const float* d_B, int flags, float* d_C) {
  GAIB_CHECK(ctx, "gaib_sgemm_split: NULL ctx");
  GAIB_CHECK(M >= 0, "gaib_sgemm_split: M < 0");
  GAIB_CHECK((flags & ~(GAIB_ACCUMULATE | GAIB_RELU)) == 0, "gaib_sgemm_split: unknown flag in %d", flags);
  if (!sgemm_split_shape_ok(ctx, N, K, lda) || (((uintptr_t)d_A | (uintptr_t)d_C) & 15) != 0 || ((uintptr_t)d_B & 3) != 0) {
    gaib_set_error("gaib_sgemm_split: not covered (4 <= K <= 256, K %% 4 == 0; 4 <= N <= 256, N %% 4 == 0; lda >= K, lda %% 4 == 0, "
                   "lda <= %lld; A and C on 16-byte boundaries; option sgemm_split_kernel = 1): N %d, K %d, lda %lld -- use gaib_sgemm_ex",
                   (long long)SS_MAX_LDA, N, K, (long long)lda);
    return GAIB_ERR_UNSUPPORTED;
  }
  if (M == 0) return GAIB_OK;
  GAIB_CHECK(d_A && d_B && d_C, "gaib_sgemm_split: NULL argument");
  GAIB_CHECK((const void*)d_A != (const void*)d_C && (const void*)d_B != (const void*)d_C, "gaib_sgemm_split: C must not alias an operand");
  SgemmSplitArgs a;
  a.A = d_A;
  a.B = d_B;
  a.C = d_C;
  a.M = M;
  a.lda = lda;
  a.N = N;
  a.K = K;
  a.transB = transB ? 1 : 0;
  a.relu = (flags & GAIB_RELU) ? 1 : 0;
  sgemm_split_grid(ctx, M, N, &a.slabs, &a.nrg);
  const int accum = (flags & GAIB_ACCUMULATE) ? 1 : 0;
  const double bytes = 4.0 * (double)M * K + 4.0 * (double)M * N * (accum ? 2.0 : 1.0) + 4.0 * (double)K * N;
  const double flops = 2.0 * (double)M * (double)N * (double)K;
  GAIB_HIP(hipSetDevice(ctx->device));
  ProfScope ps(ctx, "sgemm_split", bytes, flops, 0, SgemmSplitTag(M, N, K).s);
  switch ((K + 31) / 32) {
    case 1: return launch_sgemm_split<1>(ctx, a, accum);
    case 2: return launch_sgemm_split<2>(ctx, a, accum);
    case 3: return launch_sgemm_split<3>(ctx, a, accum);
    case 4: return launch_sgemm_split<4>(ctx, a, accum);
    case 5: return launch_sgemm_split<5>(ctx, a, accum);
    case 6: return launch_sgemm_split<6>(ctx, a, accum);
    case 7: return launch_sgemm_split<7>(ctx, a, accum);
    default: return launch_sgemm_split<8>(ctx, a, accum);
  }
}

// gaib_sgemm_ex's first route under the option sgemm_split (sgemm.hip): 1 when this call is the new kernel's
bool gaib_sgemm_split_takes(gaib_ctx* ctx, int transA, int transB, int64_t N, int64_t K, const float* d_A, const float* d_B,
                            const float* d_C) {
  return ctx->sgemm_split != 0 && !transA && N <= 256 && K <= 256 && sgemm_split_shape_ok(ctx, (int)N, (int)K, K) &&
         (((uintptr_t)d_A | (uintptr_t)d_C) & 15) == 0 && ((uintptr_t)d_B & 3) == 0 && d_A != d_C && d_B != d_C;
}
