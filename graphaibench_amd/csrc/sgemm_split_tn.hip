// sgemm_split_tn.hip -- the weight gradient C[M x N] (=|+=) A^T . G for fp32 A [K x M] and G [K x N] (K = table rows, in the
// millions; M, N <= 256) on the bf16 matrix cores with BOTH operands split exactly, sgemm_split.hip's arithmetic: an fp32 value
// is the sum of three truncated bf16 planes, the nine plane products of every term are exact in fp32 and enter an fp32
// accumulator of v_mfma_f32_16x16x32_bf16.  Optionally G <- (mask > 0 ? G : +0.0) on the way (gaib_sgemm_drelu's contract: a
// select, written back in place, the product taken of the masked G).
//
// What is different from sgemm_split.hip: the reduction index is the table row, so BOTH operands are streamed, both are split
// in flight, and both reach the matrix cores transposed (k-contiguous per column).
//
// Work.  Persistent workgroups of four waves, at most one per CU.  A workgroup owns a SLAB of up to 128 output columns (N > 128:
// two slabs, 8 workgroup ids apart -- one XCD, A's second reader) and a share of the k-steps of 32 table rows: share b of P owns
// the k-steps b, b + P, b + 2 P, ... (one compact window over K for the whole chip at any moment), P = split_tn_parts(N, K):
// K / 128 shares (four k-steps each at least: a workgroup then reads about the bytes of the partial slab it writes), at most
// num_cus / slabs.  P depends on (N, K, num_cus) alone.  P == 1 writes C itself; otherwise share b writes its columns of the
// b-th M x N slab of the workspace and split_tn_reduce_kernel sums the slabs in fixed order (old C first, slabs ascending).
// No atomics.
//
// Streaming.  Wave q takes rows 8 q .. 8 q + 7 of the k-step: per operand 8 buffer loads of 16 bytes, instruction r = row 8 q + r,
// lane l = columns 4 l .. 4 l + 3 of A, n0 + 4 l .. + 3 of G's slab on lanes 0 .. 31 -- every instruction reads one coalesced row
// segment of up to 1 KB.  After the 8 loads a lane
// holds, for each of its 4 columns, 8 k-consecutive values: component e of the 8 registers IS one MFMA fragment of column
// 4 l + e for the k-quarter q.  Rows at or past K lie behind the descriptor's end and columns at or past M / N are requested at
// SS_OUTSIDE: both arrive as zeros.  (The range check of a raw buffer covers the VGPR offset only: all of the offset is there.)
// Masked form: 8 more loads for the mask rows, one select per element, 8 buffer stores of the masked G (every element of G lies
// in one k-step of one workgroup: written once), then the split of the SELECTED registers -- a NaN behind the mask never
// reaches the planes.
//
// Split and LDS.  ss_split8 along k: three u4 per column; each is ONE 16-byte LDS write into
//     [operand][plane][16-column tile t][q][column & 15] x 16 B,     tile stride 1040 B (1024 + 16)
// so that the fragment of (operand, plane, tile) is the 1 KB at lane x 16: one conflict-free ds_read_b128.  The 16 bytes of pad
// per tile spread the WRITES: lanes 0 .. 15 of a write cover tiles l >> 2 at 64-byte steps (l & 3), 260 t + 16 c dwords, all 64
// banks once.  One k-step: 3 planes x (16 tiles of A + 8 of G's slab) x 1040 B = 74 880 B.  LDS holds ONE k-step and the double
// buffer is the registers: as soon as a wave has split its 8 + 8 rows it requests the same rows of the workgroup's next k-step
// into the registers just freed, and those loads fly under the MFMAs of the current step (288 per wave at 256 x 128, about
// 4 600 cycles, against some 500 cycles of split).  Two barriers per k-step (planes written / planes read), each behind an
// lgkmcnt(0) only: the global loads stay in flight across them.
//
// Matrix cores.  The product is taken transposed, G's fragment first: a lane ends with C[16 mt + (l & 15)][16 nt + 4 (l >> 4) + e].
// Wave w owns the row tiles MW w .. MW w + MW - 1 (MW = 1, 2, 4 for M <= 64, 128, 256) against the NT column tiles of the slab
// (4, 8 for slabs of up to 64, 128 columns): its 3 MW fragments of A stay in registers for the k-step (48 at MW = 4), every
// fragment of G read from LDS feeds 3 MW MFMAs, in groups of 12 MFMAs with the next group's fragments requested ahead.  Every
// output element lives in one accumulator register of one wave from the workgroup's first k-step to its last and takes its
// MFMAs in one order: k-steps ascending, planes of G ascending, planes of A ascending.
// Registers at MW = 4, NT = 8, masked (one wave per SIMD): 128 accumulators, 96 for the rows in flight (A, G, mask), 48 + 8 of
// fragments, the split's temporaries and addresses: 256 VGPRs + 209 AGPRs, nothing spilled.  Full-width accumulators at
// 256 x 256 (256 of them, all AGPRs) made the register allocator spill 111 - 192 VGPRs round the split: hence the slabs, and A
// read (and split) twice at N > 128.  Waves whose tiles lie past M skip the MFMAs (never the barriers).
//
// Bit identity: the k-steps of a workgroup, the slab order of the reduction and the instruction order inside a k-step are
// functions of (K, M, N, num_cus) -- two runs of one call give the same bits.
#include "split_planes.h"
#include <algorithm>

namespace {

constexpr int ST_ROWS = 32;                      // table rows of a k-step
constexpr int ST_TILE_B = 1024 + 16;             // bytes of one fragment tile in LDS (the pad spreads the writes over the banks)
constexpr int ST_SLAB = 128;                     // output columns of a workgroup: N > 128 runs as two column slabs
constexpr int ST_APLANE_B = 16 * ST_TILE_B;      // a plane of A: 16 column tiles (all of M)
constexpr int ST_GPLANE_B = 8 * ST_TILE_B;       // a plane of G: the slab's 8
constexpr int ST_AOPER_B = 3 * ST_APLANE_B;      // three planes
constexpr int ST_LDS_B = ST_AOPER_B + 3 * ST_GPLANE_B;  // A and G: 74 880 B
constexpr int ST_MIN_STEPS = 4;                  // k-steps a workgroup owns at least before K is spread over more of them

struct SplitTnArgs {
  const float* A;
  float* G;
  const float* mask;
  float* out;     // C (parts == 1) or the workspace's slabs
  int64_t K;
  int64_t slab;   // floats between the slabs of two workgroups (0: C itself)
  int M, N;
  int parts, slabs;  // workgroups along K (= slabs of the workspace summed into C), column slabs
  int accum;         // parts == 1 only: C += in the epilogue
};

// all LDS traffic of this wave has completed, then everybody's
__device__ __forceinline__ void st_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// the 8 rows a lane holds of its 4 columns -> 4 x 3 plane fragments, one 16-byte LDS write each
template <int PLANE_B>
__device__ __forceinline__ void st_split_store(const u4_t (&ld)[8], unsigned char* at) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const u4_t lo = {ld[0][e], ld[1][e], ld[2][e], ld[3][e]}, hi = {ld[4][e], ld[5][e], ld[6][e], ld[7][e]};
    u4_t p[3];
    ss_split8(lo, hi, p);
#pragma unroll
    for (int t = 0; t < 3; ++t) *reinterpret_cast<u4_t*>(at + t * PLANE_B + e * 16) = p[t];
    __builtin_amdgcn_sched_barrier(0);  // (one column's temporaries at a time)
  }
}

// a descriptor over what is left of a [K x W] fp32 array from row `row` on (at most 2^30 bytes: a k-step is 32 KB)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t st_rsrc(const float* base, int64_t row, int64_t K, int W) {
  const int64_t left = (K - row) * W * 4;
  return __builtin_amdgcn_make_buffer_rsrc((void*)(base + row * W), 0, (int)(left < (1 << 30) ? left : (1 << 30)), 0x00020000);
}

// MW: 16-row tiles of the output per wave, NT: 16-column tiles of the slab
template <int MW, int NT, bool MASK>
__global__ __launch_bounds__(256, 1) void sgemm_split_tn_kernel(SplitTnArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char st_planes[];  // A [3][16], G [3][8] tiles of ST_TILE_B
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = g.M, N = g.N;
  const int64_t K = g.K;
  const int64_t nsteps = (K + ST_ROWS - 1) / ST_ROWS;
  // workgroup -> (share b of the k-steps, column slab): the slabs of a share are 8 ids apart (one XCD: A's second reader)
  const int per = 8 * g.slabs, id = (int)blockIdx.x;
  const int n0 = ((id % per) >> 3) * ST_SLAB;
  const int64_t P = g.parts, b = (id / per) * 8 + (id & 7);
  if (b >= P) return;
  const int64_t ns = (nsteps - b + P - 1) / P;  // (P <= nsteps: every workgroup owns a k-step)

  // the loads: row 8 wv + r of the k-step, columns 4 lane .. + 3 of A, n0 + 4 lane .. + 3 of G on the lower half of the lanes
  // (M % 4 == 0, N % 4 == 0: all inside or all outside)
  const bool a_in = 4 * lane < M, g_lane = 4 * lane < ST_SLAB, g_in = g_lane && n0 + 4 * lane < N;
  const int a_v0 = (8 * wv * M + 4 * lane) * 4, g_v0 = (8 * wv * N + n0 + 4 * lane) * 4;
  // the LDS writes: tile lane >> 2, k-quarter wv, columns 4 (lane & 3) + e of the tile
  unsigned char* const wr = st_planes + (lane >> 2) * ST_TILE_B + (wv * 16 + 4 * (lane & 3)) * 16;
  // the LDS reads: lane x 16 inside the tile
  const unsigned char* const rd_a = st_planes + (MW * wv) * ST_TILE_B + lane * 16;
  const unsigned char* const rd_g = st_planes + ST_AOPER_B + lane * 16;
  const bool active = 16 * MW * wv < M;  // (wave-uniform)

  u4_t la[8], lg[8], lm[MASK ? 8 : 1];
  auto fetch = [&](int64_t s) {
    const __amdgpu_buffer_rsrc_t ra = st_rsrc(g.A, s * ST_ROWS, K, M), rg = st_rsrc(g.G, s * ST_ROWS, K, N);
#pragma unroll
    for (int r = 0; r < 8; ++r) la[r] = __builtin_amdgcn_raw_buffer_load_b128(ra, a_in ? a_v0 + r * M * 4 : SS_OUTSIDE, 0, 0);
#pragma unroll
    for (int r = 0; r < 8; ++r) lg[r] = __builtin_amdgcn_raw_buffer_load_b128(rg, g_in ? g_v0 + r * N * 4 : SS_OUTSIDE, 0, 0);
    if constexpr (MASK) {
      const __amdgpu_buffer_rsrc_t rm = st_rsrc(g.mask, s * ST_ROWS, K, N);
#pragma unroll
      for (int r = 0; r < 8; ++r) lm[r] = __builtin_amdgcn_raw_buffer_load_b128(rm, g_in ? g_v0 + r * N * 4 : SS_OUTSIDE, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);  // every load of the k-step is issued before what follows
  };

  f4 acc[MW][NT];
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[i][nt] = f4{0.f, 0.f, 0.f, 0.f};

  fetch(b);
  for (int64_t it = 0; it < ns; ++it) {
    const int64_t s = b + it * P;
    if constexpr (MASK) {  // G <- (mask > 0 ? G : +0.0), in the registers and in memory (rows past K: the store is dropped)
      const __amdgpu_buffer_rsrc_t rg = st_rsrc(g.G, s * ST_ROWS, K, N);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
#pragma unroll
        for (int e = 0; e < 4; ++e) lg[r][e] = __uint_as_float(lm[r][e]) > 0.f ? lg[r][e] : 0u;
        __builtin_amdgcn_raw_buffer_store_b128(lg[r], rg, g_in ? g_v0 + r * N * 4 : SS_OUTSIDE, 0, 0);
      }
    }
    st_split_store<ST_APLANE_B>(la, wr);
    if (g_lane) st_split_store<ST_GPLANE_B>(lg, wr + ST_AOPER_B);
    if (it + 1 < ns) fetch(s + P);  // into the registers just split, under this k-step's MFMAs
    st_barrier();                   // the planes of k-step s are in LDS
    if (active) {
      // groups of GN column tiles: 3 MW GN = 12 MFMAs per group, the next group's fragments of G requested ahead of them
      constexpr int GN = 4 / MW, NGRP = 3 * NT / GN;
      u4_t af[3][MW], gf[2][GN];
#pragma unroll
      for (int ta = 0; ta < 3; ++ta)
#pragma unroll
        for (int i = 0; i < MW; ++i) af[ta][i] = *reinterpret_cast<const u4_t*>(rd_a + ta * ST_APLANE_B + i * ST_TILE_B);
      auto read_g = [&](int grp) {  // group grp = (plane tb, column tiles nt0 .. nt0 + GN - 1), planes outermost
        const int tb = grp / (NT / GN), nt0 = (grp % (NT / GN)) * GN;
#pragma unroll
        for (int j = 0; j < GN; ++j)
          gf[grp & 1][j] = *reinterpret_cast<const u4_t*>(rd_g + tb * ST_GPLANE_B + (nt0 + j) * ST_TILE_B);
      };
      read_g(0);
#pragma unroll
      for (int grp = 0; grp < NGRP; ++grp) {
        const int nt0 = (grp % (NT / GN)) * GN;
        if (grp + 1 < NGRP) read_g(grp + 1);
#pragma unroll
        for (int ta = 0; ta < 3; ++ta)
#pragma unroll
          for (int j = 0; j < GN; ++j)
#pragma unroll
            for (int i = 0; i < MW; ++i) acc[i][nt0 + j] = ss_mfma(gf[grp & 1][j], af[ta][i], acc[i][nt0 + j]);
        __builtin_amdgcn_sched_barrier(0);  // (no further reads are pulled up: the fragments in flight stay at two groups)
      }
    }
    st_barrier();  // everybody has read the planes: the next k-step may overwrite them
  }

  // ---- epilogue: this workgroup's sums, to C or to its slab (4-byte stores: C needs no more than a float's alignment) ----
  if (!active) return;
  float* const out = g.out + b * g.slab;
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int m = 16 * (MW * wv + i) + (lane & 15), n = n0 + 16 * nt + 4 * (lane >> 4);
      if (m < M && n < N) {
        float* const o = out + (int64_t)m * N + n;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = g.accum ? o[e] + acc[i][nt][e] : acc[i][nt][e];
      }
    }
}

// C[i] = (accum ? C[i] : 0) + slab 0 [i] + slab 1 [i] + ..., in that order (sgemm.hip's splitk_reduce_kernel's rule)
__global__ void split_tn_reduce_kernel(int n, int parts, const float* slabs, int accum, float* C) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  float s = accum ? C[i] : 0.f;
#pragma unroll 8
  for (int p = 0; p < parts; ++p) s += slabs[(int64_t)p * n + i];
  C[i] = s;
}

struct SplitTnTag {
  char s[28];
  SplitTnTag(int64_t M, int64_t N, int64_t K) { snprintf(s, sizeof(s), "%lldx%lldx%lld", (long long)M, (long long)N, (long long)K); }
};

template <int MW, int NT>
int launch_split_tn(gaib_ctx* ctx, const SplitTnArgs& a) {
  const unsigned blocks = (unsigned)((a.parts + 7) / 8 * 8 * a.slabs);
  // (the attribute is set per launch, as everywhere in this library: it belongs to the function ON the current device)
  if (a.mask) {
    GAIB_HIP(hipFuncSetAttribute((const void*)sgemm_split_tn_kernel<MW, NT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    sgemm_split_tn_kernel<MW, NT, true><<<blocks, 256, ST_LDS_B, ctx->stream>>>(a);
  } else {
    GAIB_HIP(hipFuncSetAttribute((const void*)sgemm_split_tn_kernel<MW, NT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    sgemm_split_tn_kernel<MW, NT, false><<<blocks, 256, ST_LDS_B, ctx->stream>>>(a);
  }
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

template <int MW>
int launch_split_tn_n(gaib_ctx* ctx, const SplitTnArgs& a) {
  return a.N <= 64 ? launch_split_tn<MW, 4>(ctx, a) : launch_split_tn<MW, 8>(ctx, a);
}

bool split_tn_shape_ok(int64_t M, int64_t N) { return M >= 4 && M <= 256 && M % 4 == 0 && N >= 4 && N <= 256 && N % 4 == 0; }

// the launcher's grid rule: workgroups = slabs summed into each output
int64_t split_tn_parts(const gaib_ctx* ctx, int64_t N, int64_t K) {
  return std::max<int64_t>(1, std::min<int64_t>(ctx->num_cus / cdiv64(N, ST_SLAB), cdiv64(K, ST_ROWS) / ST_MIN_STEPS));
}

bool split_tn_pointers_ok(const float* d_A, const float* d_G, const float* d_mask, const float* d_C) {
  return d_A && d_G && d_C && (((uintptr_t)d_A | (uintptr_t)d_G | (uintptr_t)d_mask) & 15) == 0 && ((uintptr_t)d_C & 3) == 0 &&
         d_A != d_C && d_G != d_C && d_A != d_G && d_mask != d_C;
}

}  // namespace

extern "C" int gaib_sgemm_split_tn_cover(gaib_ctx* ctx, int64_t M, int64_t N) { return ctx && split_tn_shape_ok(M, N) ? 1 : 0; }

extern "C" int gaib_sgemm_split_tn_parts(gaib_ctx* ctx, int64_t M, int64_t N, int64_t K) {
  return ctx && split_tn_shape_ok(M, N) && K >= 1 ? (int)split_tn_parts(ctx, N, K) : 0;
}

extern "C" int gaib_sgemm_split_tn(gaib_ctx* ctx, int64_t M, int64_t N, int64_t K, const float* d_A, float* d_G,
                                   const float* d_mask, int flags, float* d_C) {
  GAIB_CHECK(ctx, "gaib_sgemm_split_tn: NULL ctx");
  if (!split_tn_shape_ok(M, N) || K < 1 || (flags & ~GAIB_ACCUMULATE) != 0 || !split_tn_pointers_ok(d_A, d_G, d_mask, d_C)) {
    gaib_set_error("gaib_sgemm_split_tn: not covered (4 <= M, N <= 256, M %% 4 == 0, N %% 4 == 0; K >= 1; A, G and mask on 16-byte "
                   "boundaries, C on a 4-byte one, no two of them the same; flags GAIB_ACCUMULATE only): M %lld, N %lld, K %lld, "
                   "flags %d -- use gaib_sgemm_ex (transA = 1) or gaib_sgemm_drelu",
                   (long long)M, (long long)N, (long long)K, flags);
    return GAIB_ERR_UNSUPPORTED;
  }
  const int accum = (flags & GAIB_ACCUMULATE) ? 1 : 0;
  const int64_t parts = split_tn_parts(ctx, N, K);
  GAIB_HIP(hipSetDevice(ctx->device));
  SplitTnArgs a;
  a.A = d_A;
  a.G = d_G;
  a.mask = d_mask;
  a.K = K;
  a.M = (int)M;
  a.N = (int)N;
  a.parts = (int)parts;
  a.slabs = (int)cdiv64(N, ST_SLAB);
  if (parts == 1) {  // one workgroup: C itself, no workspace
    a.out = d_C;
    a.slab = 0;
    a.accum = accum;
  } else {
    GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (size_t)(parts * M * N)));
    a.out = (float*)ctx->ws;
    a.slab = M * N;
    a.accum = 0;
  }
  const double bytes = 4.0 * (double)K * (double)(M + N * (d_mask ? 3 : 1)) + 4.0 * (double)(M * N) * (accum ? 2.0 : 1.0);
  const double flops = 2.0 * (double)M * (double)N * (double)K;
  ProfScope ps(ctx, "sgemm_split_tn", bytes, flops, 0, SplitTnTag(M, N, K).s);
  if (M <= 64) GAIB_TRY(launch_split_tn_n<1>(ctx, a));
  else if (M <= 128) GAIB_TRY(launch_split_tn_n<2>(ctx, a));
  else GAIB_TRY(launch_split_tn_n<4>(ctx, a));
  if (parts > 1) {
    const int n = (int)(M * N);
    split_tn_reduce_kernel<<<(unsigned)cdiv64(n, 256), 256, 0, ctx->stream>>>(n, (int)parts, (const float*)ctx->ws, accum, d_C);
    GAIB_LAUNCH_CHECK();
  }
  return GAIB_OK;
}

// the first route of gaib_sgemm_ex (transA = 1, transB = 0, no GAIB_RELU: `shape_side`) and of gaib_sgemm_drelu's masked kernel
// under the option sgemm_split_tn (sgemm.hip): true when this call is the new kernel's.  Inside a capture a workspace that would
// have to grow cannot be reserved: the route declines and the fp32 path runs.
bool gaib_sgemm_split_tn_takes(gaib_ctx* ctx, bool shape_side, int64_t M, int64_t N, int64_t K, const float* d_A, const float* d_G,
                               const float* d_mask, const float* d_C) {
  if (ctx->sgemm_split_tn == 0 || !shape_side || !split_tn_shape_ok(M, N) || K < 1 || !split_tn_pointers_ok(d_A, d_G, d_mask, d_C))
    return false;
  const int64_t parts = split_tn_parts(ctx, N, K);
  return !(ctx->capturing && parts > 1 && sizeof(float) * (size_t)(parts * M * N) > ctx->ws_bytes);
}
