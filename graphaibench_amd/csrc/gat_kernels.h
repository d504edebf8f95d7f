// gat_kernels.h -- the GAT kernels that more than one translation unit instantiates: the one-sweep forward and backward
// (chunk kernels, the packed-math sweep, their reductions), the per-vertex dots and the alpha-gradient reduction, with the
// shape rules and dispatch macros of their callers.  The host sequences that launch the one-sweep kernels are gat_fused_seq.h,
// included by gat_fused.hip (fp32 tables: the plain, DROP, WIDE and WIN forms) and by gat_bf16.hip (element type E = uint16_t:
// raw bf16 bits, loaded as they are and widened where they are consumed); gat.hip holds the staged path.
// DROP: attention dropout inside the two sweeps.
// WIDE: rows of a table whose row stride is not the row width (one column slab of a wider multi-head row) -- a template flag with
// trailing, defaulted stride arguments read only behind `WIDE ? ld : len`: the other instantiations compile to the instructions
// they had (the arguments sit behind every argument those read).
// WIN (the dropped sweeps on a slab): the dropout mask's index takes the FULL row's head count and the slab's first head from
// two more trailing arguments (gat_drop_bits); forward: DROP && WIDE, backward: a template flag of its own.
#pragma once
#include "common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- element type of the gathered tables: E = float, or uint16_t = raw bf16 bits (gat_bf16.hip) ---------------------------
// A lane's four columns of a row travel and wait in registers AS LOADED (Raw: 16 bytes of fp32, 8 bytes of bf16) and are widened
// where they are consumed, behind the batch's sched_barrier: a shift / a mask per element, exact.  For E = float widen() is the
// identity and the kernels below are the fp32 kernels as they were.
template <typename E>
struct Row4;
template <>
struct Row4<float> {
  typedef f4 Raw;
  static __device__ __forceinline__ f4 widen(const f4& r) { return r; }
};
template <>
struct Row4<uint16_t> {
  typedef u32x2 Raw;
  static __device__ __forceinline__ f4 widen(const u32x2& r) {
    return f4{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16),
              __uint_as_float(r[1] & 0xffff0000u)};
  }
};
template <typename E>
__device__ __forceinline__ typename Row4<E>::Raw load_row4(const E* p) {
  return *reinterpret_cast<const typename Row4<E>::Raw*>(p);
}
__device__ __forceinline__ float elem_f32(float v) { return v; }
__device__ __forceinline__ float elem_f32(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

// partial[b][0][c] = sum_{v in strip b} rs[v, head(c)]*x[v][c]; partial[b][1][c] likewise with cs.
// 256 threads: thread t owns column (t % cw) of every (256/cw)-th row of the strip.
// WIDE: x has rows of ld elements (>= len); rs, cs and partial are the slab's own
template <typename E, bool WIDE = false>
__global__ __launch_bounds__(256) void alpha_partial_kernel(int64_t nv, int len, int H, const E* x,
                                                            const float* rs, const float* cs,
                                                            int64_t rows_per_block, float* partial, int ld = 0) {
  const int xld = WIDE ? ld : len;
  extern __shared__ float sm[];  // [2][256]
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < nv) ? r0 + rows_per_block : nv;
  float* out = partial + (int64_t)blockIdx.x * 2 * len;
  const int dh = len / H;
  for (int c0 = 0; c0 < len; c0 += 256) {
    const int cw = (len - c0 < 256) ? (len - c0) : 256;  // columns in this pass
    const int rpp = 256 / cw;                            // rows per pass (>=1)
    const int tc = threadIdx.x % cw, tr = threadIdx.x / cw;
    const int hd = (c0 + tc) / dh;
    float al = 0.f, ar = 0.f;
    if (tr < rpp) {
      for (int64_t v = r0 + tr; v < r1; v += rpp) {
        const float xv = elem_f32(x[v * (int64_t)xld + c0 + tc]);
        al += rs[v * H + hd] * xv;
        ar += cs[v * H + hd] * xv;
      }
    }
    sm[threadIdx.x] = (tr < rpp) ? al : 0.f;
    sm[256 + threadIdx.x] = (tr < rpp) ? ar : 0.f;
    __syncthreads();
    if (threadIdx.x < cw) {
      float sl_ = 0.f, sr_ = 0.f;
      for (int k = 0; k < rpp; ++k) {
        sl_ += sm[k * cw + threadIdx.x];
        sr_ += sm[256 + k * cw + threadIdx.x];
      }
      out[c0 + threadIdx.x] = sl_;
      out[len + c0 + threadIdx.x] = sr_;
    }
    __syncthreads();
  }
}

// one wave per output element (column c of lgrad or rgrad): lanes stride over the block partials, then a fixed-order
// wave sum (one thread per column walked 1024 partials serially: 0.25 ms of pure latency)
__global__ __launch_bounds__(256) void alpha_final_kernel(int nblocks, int len, const float* partial, float* lgrad,
                                                          float* rgrad) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);  // [0, 2 * len)
  if (w >= 2 * len) return;
  const int lane = threadIdx.x & 63;
  float s = 0.f;
  for (int b = lane; b < nblocks; b += 64) s += partial[(int64_t)b * 2 * len + w];
  s = wave_sum(s);
  if (lane == 0) (w < len ? lgrad : rgrad)[w < len ? w : w - len] = s;
}

// rowdot[v,h] = <a[v, slice h], b[v, slice h]>.  One wave per row.  WIDE: a and b have rows of ld elements; out stays [nv][H]
template <typename E, bool WIDE = false>
__global__ __launch_bounds__(256) void rowdot_kernel(int64_t nv, int len, int H, const E* a,
                                                     const float* b, float* out, int ld = 0) {
  const int xld = WIDE ? ld : len;
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const E* ar = a + row * (int64_t)xld;
  const float* br = b + row * (int64_t)xld;
  const int dh = len / H;
  if (H > 1 && dh <= 64 && (64 % dh) == 0) {  // as in vertex_dots_kernel
    for (int c0 = 0; c0 < len; c0 += 64) {
      const int c = c0 + lane;
      const bool ok = c < len;
      float s = ok ? elem_f32(ar[c]) * br[c] : 0.f;
      for (int o = dh >> 1; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
      if (ok && (lane % dh) == 0) out[row * H + c / dh] = s;
    }
    return;
  }
  for (int h = 0; h < H; ++h) {
    float s = 0.f;
    for (int c = h * dh + lane; c < (h + 1) * dh; c += 64) s += elem_f32(ar[c]) * br[c];
    s = wave_sum(s);
    if (lane == 0) out[row * H + h] = s;
  }
}

// rec[v, h] = (rowdot[v, h], row maximum, 1 / row sum, 0): what the one-sweep backward needs about a COLUMN vertex beside
// its two rows, as one 16-byte record -- 128 B = one line per vertex at 8 heads, where rowdot [nv][H] and the forward's
// statistics [nv][H][2] were two tables, two lines and two load instructions per edge
__global__ void gat_rec_kernel(int64_t n, const float* rowdot, const float2* stats, f4* rec) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    const float2 st = stats[t];
    rec[t] = f4{rowdot[t], st.x, st.y, 0.f};
  }
}

// ---- lane layout of the one-sweep kernels, by row width (round 5: len = 32, 64 and 128) -------------------------------
// A lane owns 4 columns of a row, so a row takes G = len / 4 lanes (8, 16, 32) and a wave works on NG = 64 / G edges at a
// time, G steps per 64-edge chunk.  The chunk's column ids are fetched ONCE, one or two per lane, laid out so that "the
// column of (my group, step t)" is a row-share DPP inside the lane's 16-lane row (no LDS, no bpermute):
//   G = 16: 4 groups = the 4 DPP rows.  Lane (row r, position p) holds edge p*4 + r; (group r, step t) = edge t*4 + r.
//   G =  8: 8 groups, two per DPP row (half hg = 0, 1).  Same holding; (group (r, hg), step t) = edge (2t + hg)*4 + r:
//           two row-shares with constant lane numbers and a select on hg.
//   G = 32: 2 groups of two DPP rows.  (group g, step t) = edge t*2 + g; every lane of the group's two rows holds TWO ids,
//           edges p*2 + g and (p + 16)*2 + g (both rows load the same lines), so steps 0..15 come from the first, 16..31
//           from the second.
// In every layout the edges of step t are t*NG .. t*NG + NG - 1: a chunk of n edges takes ceil(n / NG) steps.
template <int G>
struct ChunkLanes {
  static_assert(G == 8 || G == 16 || G == 32, "len = 32, 64 or 128");
  static constexpr int NG = 64 / G;
  // the edge whose id this lane holds (which = 1: the second one, G = 32 only)
  static __device__ __forceinline__ int held_edge(int lane, int which) {
    const int r = lane >> 4, p = lane & 15;
    if constexpr (G == 32) return (p + 16 * which) * 2 + (r >> 1);
    else return p * 4 + r;
  }
  // the edge of (this lane's group, step t)
  static __device__ __forceinline__ int step_edge(int lane, int t) {
    if constexpr (G == 32) return t * 2 + (lane >> 5);
    else if constexpr (G == 16) return t * 4 + (lane >> 4);
    else return (2 * t + ((lane >> 3) & 1)) * 4 + (lane >> 4);
  }
  // its held value (a column id, a reverse-edge id): t is a compile-time constant after unrolling
  static __device__ __forceinline__ int step_value(int v0, int v1, int lane, int t) {
    if constexpr (G == 32) return t < 16 ? row_lane(v0, t) : row_lane(v1, t - 16);
    else if constexpr (G == 16) return row_lane(v0, t);
    else {
      const int a = row_lane(v0, 2 * t), b = row_lane(v0, 2 * t + 1);
      return ((lane >> 3) & 1) ? b : a;
    }
  }
};
// lanes_sum over an aligned group of up to 32 lanes (LH = 32: one head over a 128-wide row)
template <int LH>
__device__ __forceinline__ float lanes_sum_w(float v) {
  if constexpr (LH <= 16) return lanes_sum<LH>(v);
  else {
    v = lanes_sum<16>(v);
    return v + __shfl_xor(v, 16, 64);
  }
}

// ---- the whole edge side of GAT backward in ONE pass over the ordered 64-edge chunk list ---------------------------
// GAT_Aggregator::d_aggregate (gat_aggregator.cpp:99-200) is four sweeps over the edges: SDDMM dp_e = <grad_i, h_c>;
// softmax backward + leaky-relu' -> g_e, with the row sums rs and the column sums cs of g for the alpha gradients;
// the transpose pT_e = p[rev e]; the aggregation out_i = sum_e pT_e grad_c.  Staged (the kernels above) they move
// ~340 B per edge through HBM at 8 heads (dp written and read twice, (g, p) records written and re-read through rev,
// pT written and read).  Everything a row needs about its edge e = (i -> c) and the reverse edge (c -> i) follows from
// per-vertex quantities and ONE attention value each:
//   dp_e  = <grad_i, h_c>        g_e  = f(p_e,  dp_e,  rowdot_i, sl_i + sr_c)     -> rs_i += g_e
//   dp_r  = <grad_c, h_i>        g_r  = f(p_r,  dp_r,  rowdot_c, sl_c + sr_i)     -> cs_i += g_r   (p_r = p[rev e])
//   out_i += p_r * grad_c
// with rowdot_v = <grad_v, forward output_v> = sum_e p_e dp_e of row v (the one-pass form of softmax_bwd_v2_kernel) and
// f(p, dp, dot, t) = (p (1 - p) dp - (dot - p dp) p) * (t > 0 ? 1 : eps).  So one sweep gathers the rows h_c and grad_c
// (the two gathers SDDMM and the aggregation did separately), reads p_e (linear) and p_r (one random 4H-byte access),
// and writes nothing per edge: ~4 + 4 + 4H + 4H bytes per edge through HBM next to the two cache-resident row gathers.
// Chunk by chunk in column-block order like sddmm_chunk_kernel / spmm_chunk_kernel (rows in flight gather from one
// window of the tables); per chunk a partial output row and partial rs / cs, added per row in chunk order by
// gat_fused_reduce_kernel: deterministic, no atomics.
//
// Lanes: group k = lane / G owns edges k*G .. k*G+G-1 of the chunk, lane sl = lane % G owns 4 columns (head = sl / LH,
// LH = G / H lanes per head).  EVERYTHING is fetched in that layout, U edges per group in flight: the two rows (16 B per
// lane), rowdot of the column vertex and the two attention values p_e, p_r (4 B each), so the only dependent step is
// col / rev -> gathers, as in spmm_chunk_kernel.  A first version kept the per-(edge, head)
// scalars one EDGE per lane (H-vectors) and met the column layout through LDS: 64 different lines per wave instruction
// for each of five H-vector fetches, a dependent post-phase and 178 -> 142 VGPRs made it 10.5 ms at the reddit shape
// against 12.3 ms for the staged kernels.
// RECOMP: the attention values are not read but formed again from the forward sweep's row statistics
// (gat_fwd_fused_chunk_kernel): p_e = exp(lrelu(sl_i + sr_c) - M_i) / S_i and p_r = exp(lrelu(sl_c + sr_i) - M_c) / S_c
// with stats[v][h] = (M, 1/S) -- one 8-B gather from a 15 MB table instead of 4 B linear + 4 B random + rev per edge, and
// no [ne][H] array exists at all.
// T[v] = [h_v (len) | grad_v (len) | rec_v (4 H)]: what the backward sweep gathers per edge, as ONE row per vertex
__global__ __launch_bounds__(256) void gat_interleave_kernel(int64_t nv, int len4, int H, const f4* feat, const f4* grad,
                                                             const f4* rec, f4* T) {
  const int ldt4 = 2 * len4 + H;
  const int64_t total = nv * ldt4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t v = i / ldt4;
    const int k = (int)(i - v * ldt4);
    T[i] = k < len4 ? feat[v * len4 + k] : (k < 2 * len4 ? grad[v * len4 + k - len4] : rec[v * H + k - 2 * len4]);
  }
}

// ---- attention dropout inside the one-sweep kernels (DROP; gat_drop.hip) ---------------------------------------------------
// w_(e,k) = mask . scale with mask = u01(seed, e * H + k) > rate: the mask gaib_dropout draws for element e * H + k of an
// [ne][H] array under the same seed (e: the edge's position in the CSR, k: the head), formed here instead of read -- no edge
// array exists.  A 64-bit splitmix per lane and step would be redundant over the LH lanes of a head and costs more than the
// step it gates (the sweeps are VALU-bound), so a chunk's masks are formed ONCE, ahead of the edge loop: the LH lanes of a
// head share its G steps -- lane q of the head takes steps q, q + LH, ... (H hashes per lane instead of G), one bit per
// step, and an OR over the head's lanes (DPP) leaves all G bits in each of them.  In the loop the mask of step t is bit t.
// IDS = false: the chunk's own edges eb + (edge of the step) -- consecutive steps of a lane are LH * NG edges apart, so the
// key of the next step is an addition; else the ids are read from ids[] at those positions (the reverse edges).
// WIN: the chunk is one column slab of a wider row -- H heads from head mask_head0 on of mask_heads: the mask is the one of element
// e * mask_heads + mask_head0 + k of the virtual [ne][mask_heads] array (e * H + k would be another mask).  The key is linear in
// the index, so the slab needs those two numbers and nothing else; the row side's step increment becomes one wave-uniform 64-bit
// product per chunk, U01_GOLD (LH NG) mask_heads, where the other form folds a constant.
// (the two arguments are read under WIN only)
template <int G, int H, bool IDS, bool WIN>
__device__ __forceinline__ uint32_t gat_drop_bits(int lane, int n, int64_t eb, const uint32_t* ids, uint64_t seed, float rate,
                                                  int mask_heads, int mask_head0) {
  constexpr int LH = G / H;
  using CL = ChunkLanes<G>;
  constexpr int NG = CL::NG;
  const int sl = lane & (G - 1);
  const int head = sl / LH, q = sl & (LH - 1);
  const int e0 = CL::step_edge(lane, q);  // step t of this lane's group is edge e0 + (t - q) * NG
  uint64_t z, dz, mh, hd;                 // key, its increment per step of this lane, row length and column of the mask array
  if constexpr (WIN) {
    mh = (uint64_t)mask_heads;
    hd = (uint64_t)mask_head0 + (uint64_t)head;
    dz = (U01_GOLD * (uint64_t)(LH * NG)) * mh;
  } else {
    mh = (uint64_t)H;
    hd = (uint64_t)head;
    dz = U01_GOLD * (uint64_t)(LH * NG * H);
  }
  z = u01_key(seed, (uint64_t)(eb + e0) * mh + hd);  // (the index in 64 bits: ne * H passes 2^32)
  uint32_t bits = 0;
#pragma unroll
  for (int s = 0; s < H; ++s) {  // step s * LH + q
    if (s * LH * NG < n) {       // (wave-uniform: else no lane's step s * LH + q has an edge)
      if constexpr (IDS) {
        const int ei = e0 + s * LH * NG;
        z = u01_key(seed, (uint64_t)ids[eb + (ei < n ? ei : 0)] * mh + hd);
      }
      bits |= (u01_of_key(z) > rate ? 1u : 0u) << (s * LH + q);
      if constexpr (!IDS) z += dz;
    }
  }
  return lanes_or<LH>(bits);
}

// DROP (RECOMP form): attention dropout inside the sweep, see gat_drop_bits; rev is then read for the reverse edges' masks.
// The three trailing arguments are the DROP form's; the others' launches leave them to their defaults.
// WIN (DROP form): the masks' index window, see gat_drop_bits; its two arguments trail the DROP form's.
template <int G, int H, int U, bool RECOMP, typename E, bool DROP = false, bool WIN = false>
__global__ __launch_bounds__(256) void gat_bwd_fused_chunk_kernel(
    int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase, const uint32_t* chunk_start,
    const int64_t* rowptr, const uint32_t* col, const uint32_t* rev, int len, const E* feat, const E* grad,
    const float* p, const float2* stats, const float* rowdot, const float* alpha_l, const float* alpha_r, float eps,
    float* out_partial, float* rc_partial, const f4* rec, int phase, uint32_t own_cols, int ld, int rec_ld, int per_xcd,
    float drop_rate = 0.0f, float drop_scale = 1.0f, uint64_t drop_seed = 0, int mask_heads = 0, int mask_head0 = 0) {
  static_assert(!WIN || DROP, "the head window belongs to the dropout mask");
  // rec (RECOMP): (rowdot, row maximum, 1 / row sum) per (vertex, head) as one 16-byte record, see gat_rec_kernel
  // ld / rec_ld: row strides of the feat / grad tables (floats) and of the record table (16-byte records): len and H for
  // three separate tables; 2 len + 4 H and that / 4 when the three live INTERLEAVED, one [h | grad | records] row per vertex
  // (gat_interleave_kernel) -- one contiguous 640-B region per edge instead of three.
  // per_xcd > 0: workgroups are dealt to the XCDs round robin (XCD = blockIdx & 7); XCD x then walks the CONTIGUOUS range
  // [x per_xcd, (x + 1) per_xcd) of the column-block-ordered chunk list, so each L2 sees its own eighth of the columns
  // instead of all eight L2s caching the same window.
  constexpr int LH = G / H;  // lanes per head
  using CL = ChunkLanes<G>;
  constexpr int NG = CL::NG;
  int64_t blk = blockIdx.x;
  if (per_xcd > 0) blk = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  const int64_t c = blk * 4 + (threadIdx.x >> 6);
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const int sl = lane & (G - 1), gbase = lane & ~(G - 1);
  const int64_t row = chunk_row[c];
  const int64_t eb = chunk_ebase[c];
  const int64_t rb = rowptr[row];
  const int64_t rem = rowptr[row + 1] - eb;
  const int n = rem < 64 ? (int)rem : 64;

  // step t of lane group g is edge t * NG + g (ChunkLanes): a chunk of n edges takes ceil(n / NG) steps whatever n is (with
  // group g on edges 16 g .. 16 g + 15, the 17-edge tail of a row took all 16).  The lanes fetch the chunk's column ids
  // once, laid out so that "the column of my group's step t" is a DPP row-share.
  const int my_e = CL::held_edge(lane, 0), my_e1 = CL::held_edge(lane, 1);
  const int64_t el = eb + (my_e < n ? my_e : 0);
  const uint32_t cl = col[el];
  uint32_t cl1 = 0;
  int64_t el1 = eb;
  if constexpr (G == 32) {
    el1 = eb + (my_e1 < n ? my_e1 : 0);
    cl1 = col[el1];
  }
  // a rank's rows over [owned | halo] columns (a row keeps the global edge order, so halo ids sit on both sides of the
  // owned ones): phase 0 sweeps the chunks that touch owned columns only -- while the halo rows are still on the wire --,
  // phase 1 the others; -1: all
  if (phase >= 0 && ((__ballot((my_e < n && cl >= own_cols) || (G == 32 && my_e1 < n && cl1 >= own_cols)) == 0) != (phase == 0))) return;
  uint32_t rl = 0, rl1 = 0;
  if constexpr (!RECOMP) {
    rl = rev[el];
    if constexpr (G == 32) rl1 = rev[el1];
  }
  // DROP: the masks of the chunk's edges (-> dp_e) and of their reverse edges (-> dp_r, the weight of grad_c), one bit per step
  uint32_t mb_e = 0, mb_r = 0;
  if constexpr (DROP) {
    mb_e = gat_drop_bits<G, H, false, WIN>(lane, n, eb, nullptr, drop_seed, drop_rate, mask_heads, mask_head0);
    mb_r = gat_drop_bits<G, H, true, WIN>(lane, n, eb, rev, drop_seed, drop_rate, mask_heads, mask_head0);
  }
  const int coff = sl * 4;  // len == 4 * G
  const int head = sl / LH;
  using R4 = Row4<E>;
  const f4 gi = R4::widen(load_row4(grad + row * (int64_t)ld + coff));
  const f4 hi = R4::widen(load_row4(feat + row * (int64_t)ld + coff));
  // the per-vertex dots a_l.h_v, a_r.h_v are formed again from the gathered rows (4 FMAs + the head's shuffle each)
  // instead of being gathered: only rowdot, which needs the vertex's forward output, comes from a table -- [nv][H]
  // floats, small enough for the L2, where a (rowdot, sl, sr) record per (vertex, head) cost a 128-B line per edge
  const f4 al4 = *reinterpret_cast<const f4*>(alpha_l + coff);
  const f4 ar4 = *reinterpret_cast<const f4*>(alpha_r + coff);
  // (instruction count is what bounds this kernel -- 2 000 VALU / LDS instructions per 64-edge chunk, 1 720 chunks per
  // SIMD: 5.7 ms of issue at the reddit shape before a byte moves -- so: dot products as FMA chains, sums over a head's
  // lanes and "column id of edge j" by DPP instead of ds_bpermute, one fast exponential per attention value)
  auto d4 = [](const f4& a, const f4& b) {
    return __builtin_fmaf(a[3], b[3], __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0])));
  };
  const float sl_i = lanes_sum_w<LH>(d4(al4, hi));
  const float sr_i = lanes_sum_w<LH>(d4(ar4, hi));
  float rd_i;
  float2 st_i = {0.f, 0.f};
  if constexpr (RECOMP) {
    const f4 ri = rec[row * rec_ld + head];
    rd_i = ri[0];
    st_i = float2{ri[1], ri[2]};
  } else {
    rd_i = rowdot[row * H + head];
  }
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  float s_e = 0.f, s_r = 0.f;
#pragma unroll
  for (int j = 0; j < G; j += U) {
    if (j * NG >= n) break;  // (wave-uniform: no edge of the chunk is left for any group)
    typename R4::Raw xg_raw[U], xh_raw[U];
    float pe[U], pr[U], rd[U];
    float2 stc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ei = CL::step_edge(lane, j + u);
      const uint32_t cj = (uint32_t)CL::step_value((int)cl, (int)cl1, lane, j + u);
      xg_raw[u] = load_row4(grad + (int64_t)cj * ld + coff);
      xh_raw[u] = load_row4(feat + (int64_t)cj * ld + coff);
      if constexpr (RECOMP) {
        const f4 rc = rec[(int64_t)cj * rec_ld + head];
        rd[u] = rc[0];
        stc[u] = float2{rc[1], rc[2]};
      } else {
        rd[u] = rowdot[(int64_t)cj * H + head];
        const uint32_t rj = (uint32_t)CL::step_value((int)rl, (int)rl1, lane, j + u);
        pe[u] = p[(eb + (ei < n ? ei : 0)) * H + head];
        pr[u] = p[(int64_t)rj * H + head];
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // all loads of the batch are issued before the first one is consumed
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = CL::step_edge(lane, j + u) < n;
      const f4 xg = R4::widen(xg_raw[u]), xh = R4::widen(xh_raw[u]);
      float dpe = lanes_sum_w<LH>(d4(gi, xh));
      float dpr = lanes_sum_w<LH>(d4(xg, hi));
      float w_r = 1.0f;
      if constexpr (DROP) {  // d(out_i)/d(p_e) = w_e <grad_i, h_c>; the same through the reverse edge's mask on the column side
        dpe *= ((mb_e >> (j + u)) & 1u) ? drop_scale : 0.0f;
        w_r = ((mb_r >> (j + u)) & 1u) ? drop_scale : 0.0f;
        dpr *= w_r;
      }
      const float sl_c = lanes_sum_w<LH>(d4(al4, xh));
      const float sr_c = lanes_sum_w<LH>(d4(ar4, xh));
      const float t_e = sl_i + sr_c, t_r = sl_c + sr_i;  // pre-activation scores of (i -> c) and (c -> i)
      float a, b;
      if constexpr (RECOMP) {
        a = __expf((t_e > 0.0f ? t_e : eps * t_e) - st_i.x) * st_i.y;
        b = __expf((t_r > 0.0f ? t_r : eps * t_r) - stc[u].x) * stc[u].y;
      } else {
        a = pe[u];
        b = pr[u];
      }
      const float dse = a * (1.0f - a) * dpe - (rd_i - a * dpe) * a;
      const float dsr = b * (1.0f - b) * dpr - (rd[u] - b * dpr) * b;
      const float ge = dse * (t_e > 0.0f ? 1.0f : eps);  // leaky-relu' at the score of (i -> c)
      const float gr = dsr * (t_r > 0.0f ? 1.0f : eps);  //              at the score of (c -> i)
      if (live) {  // (lanes past the end of a short chunk looked at the chunk's first edge: nothing of it is added)
        s_e += ge;
        s_r += gr;
        if constexpr (DROP) {  // the gradient flows back along the DROPPED attention p_r w_r
          const float bw = b * w_r;
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(bw, xg[k], acc[k]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(b, xg[k], acc[k]);
        }
      }
    }
  }
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
    s_e += __shfl_xor(s_e, o, 64);
    s_r += __shfl_xor(s_r, o, 64);
  }
  const int64_t slot = (int64_t)chunk_start[row] + (eb - rb) / 64;
  if (gbase == 0) {
    *reinterpret_cast<f4*>(out_partial + slot * len + coff) = acc;
    if ((sl & (LH - 1)) == 0) {
      rc_partial[slot * 2 * H + head] = s_e;      // partial row sum of g    (-> alpha_l gradient)
      rc_partial[slot * 2 * H + H + head] = s_r;  // partial column sum of g (-> alpha_r gradient)
    }
  }
}

// ---- the same sweep on a VALU diet (round 6) ----------------------------------------------------------------------------
// Counters of gat_bwd_fused_chunk_kernel<16, 8, 4, true> at the reddit shape (profiles/r06/gat_bwd_sq.json): 2.48 G VALU
// instructions per launch = 1 324 per 64-edge chunk, SQ_ACTIVE_INST_VALU = 2.53 G quad-cycles -- 4.1 ms of pure VALU issue on
// 1 024 SIMDs at 2.4 GHz, which IS the 4.4-4.7 ms the sweep takes with every gather served by the L2 (gat_l2_ceiling.py):
// the kernel is VALU-bound.  Its ISA shows where the instructions go: hipcc packs the e-side and the r-side chains into
// v_pk_*_f32 pairs, and 461 of the 1 389 VALU instructions are v_mov_b32 marshalling operands into aligned register pairs;
// the sums over a head's lanes are v_mov_b32_dpp + add (the packed add cannot take a DPP operand) behind a zero-initialising
// move each; three 64-bit row addresses per edge cost a v_mad_u64_u32 + v_lshl_add_u64 each.  Here the data layout makes the
// pairs natural instead:
//   * the table row of a vertex interleaves h and grad ELEMENT by element: lane sl reads (h0 g0 h1 g1 | h2 g2 h3 g3), so
//     (h_k, g_k) is an aligned register pair as loaded;
//   * chain P = (dpe, dpr) = sum_k (grad_i[k], h_i[k]) * (h_c[k], grad_c[k]) and chain Q = (sr_c, sl_c) = sum_k (a_r[k], a_l[k]) *
//     (h_c[k], h_c[k]) are four packed multiply-adds each, in d4()'s order of additions (same bits), with loop-invariant left
//     operands; (t_e, t_r) = (sl_i, sr_i) + Q and everything downstream stays in pairs without a move;
//   * the sums over a head's lanes are v_add_f32_dpp, one instruction per value and stage (inline: the compiler does not fold a
//     DPP move into an add whose other operand is not the identity);
//   * one 32-bit byte offset per edge addresses all three loads of its row (tables below 4 GB; else the kernel above);
//   * the softmax backward in its short form g = p (dp - rowdot) -- the reference's p (1 - p) dp - (rowdot - p dp) p
//     (math_functions.cpp:496-514) multiplied out; one rounding fewer per term, not the same bits.
// ~41 VALU instructions per edge step instead of ~80 (898 against 1 389 in the kernel's ISA at 8 heads x 8).  RECOMP form only
// (the attention is formed again from the row statistics), heads of at most 16 lanes.
// MEASURED (reddit shape, 8 heads x 8, scripts/gat_l2_ceiling.py, profiles/r06/gat_pk_*): with every gather served by the L2
// (column ids >> 8) the backward call drops from 4.31 to 3.95 ms -- and at the REAL column ids it does not move: 6.27 against
// 6.25 ms.  There the sweep draws 43 GB per launch through the L2 -> fabric boundary at 7 TB/s (0.82 of the cache-resident gather
// rate, L2 hit rate 0.42): the VALU work had been hiding under the gathers all along.  So the kernel is an OPTION (gat_bwd_pk = 1),
// off by default -- it costs the table build (0.06 ms at the reddit shape, 0.45 ms at the products shape) and buys nothing where
// the tables do not fit the L2s; tests/test_gpu_ops.py runs both.
typedef float f2 __attribute__((ext_vector_type(2)));

// T2[v] = [(h0 g0 h1 g1 ...) 2 len | records 4 H]: h and grad of vertex v element by element, then its (rowdot, M, 1/S, 0) records
__global__ __launch_bounds__(256) void gat_interleave_pairs_kernel(int64_t nv, int len4, int H, const f4* feat, const f4* grad,
                                                                   const f4* rec, f4* T) {
  const int ldt4 = 2 * len4 + H;
  const int64_t total = nv * ldt4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t v = i / ldt4;
    const int k = (int)(i - v * ldt4);
    if (k < 2 * len4) {
      const f4 h = feat[v * len4 + (k >> 1)], g = grad[v * len4 + (k >> 1)];
      T[i] = (k & 1) ? f4{h[2], g[2], h[3], g[3]} : f4{h[0], g[0], h[1], g[1]};
    } else {
      T[i] = rec[v * H + k - 2 * len4];
    }
  }
}

// a, b, c, d <- their sums over the aligned group of LH lanes (LH = 1 .. 16 inside a 16-lane row); every lane gets them.
// v_add_f32_dpp reads its permuted operand through the DPP path: a VGPR written by the VALU instruction right before needs two
// wait states there, and the compiler's hazard recogniser does not look inside inline assembly -- hence the leading s_nop; the
// later stages read registers written four instructions earlier.
template <int LH>
__device__ __forceinline__ void lanes_sum4_dpp(float& a, float& b, float& c, float& d) {
  static_assert(LH == 1 || LH == 2 || LH == 4 || LH == 8 || LH == 16, "aligned power-of-two groups inside a 16-lane row");
#define GAIB_DPP4(CTRL)                                                                   \
  asm volatile("s_nop 1\n\t"                                                               \
               "v_add_f32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf\n\t"          \
               "v_add_f32_dpp %1, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf\n\t"          \
               "v_add_f32_dpp %2, %2, %2 " CTRL " row_mask:0xf bank_mask:0xf\n\t"          \
               "v_add_f32_dpp %3, %3, %3 " CTRL " row_mask:0xf bank_mask:0xf"              \
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
  if constexpr (LH >= 2) GAIB_DPP4("quad_perm:[1,0,3,2]");
  if constexpr (LH >= 4) GAIB_DPP4("quad_perm:[2,3,0,1]");
  if constexpr (LH >= 8) GAIB_DPP4("row_half_mirror");
  if constexpr (LH >= 16) GAIB_DPP4("row_mirror");
#undef GAIB_DPP4
}

// A lane's four (h_k, g_k) pairs of a packed-math table row as they travel: two 16-byte loads of fp32 (h0 g0 h1 g1 | h2 g2 h3 g3),
// or ONE of bf16 -- dword k holds h_k in its low half and g_k in its high half (gat_pairs_bf16_kernel) --, widened into the same
// four register pairs where they are consumed.  Row of a vertex: DW * len dwords of pairs, then its fp32 records (16 H bytes).
template <typename E>
struct Pair4;
template <>
struct Pair4<float> {
  struct Raw { f4 a, b; };
  static constexpr uint32_t BYTES = 32u;  // of a lane's four pairs
  static constexpr int DW = 2;             // dwords per column in a row
  static __device__ __forceinline__ Raw load(const char* Tb, uint32_t off) {  // (32-bit byte offsets: tables below 4 GB)
    return Raw{*reinterpret_cast<const f4*>(Tb + (size_t)off), *reinterpret_cast<const f4*>(Tb + (size_t)(off + 16u))};
  }
  static __device__ __forceinline__ void widen(const Raw& r, f2& e0, f2& e1, f2& e2, f2& e3) {
    e0 = f2{r.a[0], r.a[1]}; e1 = f2{r.a[2], r.a[3]}; e2 = f2{r.b[0], r.b[1]}; e3 = f2{r.b[2], r.b[3]};
  }
};
template <>
struct Pair4<uint16_t> {
  typedef u32x4 Raw;
  static constexpr uint32_t BYTES = 16u;
  static constexpr int DW = 1;
  static __device__ __forceinline__ Raw load(const char* Tb, uint32_t off) { return *reinterpret_cast<const u32x4*>(Tb + (size_t)off); }
  static __device__ __forceinline__ void widen(const Raw& r, f2& e0, f2& e1, f2& e2, f2& e3) {
    e0 = f2{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u)};
    e1 = f2{__uint_as_float(r[1] << 16), __uint_as_float(r[1] & 0xffff0000u)};
    e2 = f2{__uint_as_float(r[2] << 16), __uint_as_float(r[2] & 0xffff0000u)};
    e3 = f2{__uint_as_float(r[3] << 16), __uint_as_float(r[3] & 0xffff0000u)};
  }
};

// T2 of bf16 tables: [len dwords (g_k << 16 | h_k) | records 4 H floats] per vertex, 16 bytes per thread
__global__ __launch_bounds__(256) void gat_pairs_bf16_kernel(int64_t nv, int len4, int H, const u32x2* feat, const u32x2* grad,
                                                             const f4* rec, u32x4* T) {
  const int ldt4 = len4 + H;
  const int64_t total = nv * ldt4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t v = i / ldt4;
    const int k = (int)(i - v * ldt4);
    if (k < len4) {
      const u32x2 h = feat[v * len4 + k], g = grad[v * len4 + k];
      T[i] = u32x4{(h[0] & 0xffffu) | (g[0] << 16), (h[0] >> 16) | (g[0] & 0xffff0000u), (h[1] & 0xffffu) | (g[1] << 16),
                   (h[1] >> 16) | (g[1] & 0xffff0000u)};
    } else {
      const f4 r = rec[v * H + k - len4];
      T[i] = u32x4{__float_as_uint(r[0]), __float_as_uint(r[1]), __float_as_uint(r[2]), __float_as_uint(r[3])};
    }
  }
}

template <int G, int H, int U, typename E>
__global__ __launch_bounds__(256) void gat_bwd_fused_pk_kernel(int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase,
                                                               const uint32_t* chunk_start, const int64_t* rowptr, const uint32_t* col,
                                                               int len, const E* T, const float* alpha_l, const float* alpha_r,
                                                               float eps, float* out_partial, float* rc_partial, int per_xcd) {
  constexpr int LH = G / H;  // lanes per head
  static_assert(LH <= 16, "a head's lanes sit inside one 16-lane DPP row");
  using CL = ChunkLanes<G>;
  constexpr int NG = CL::NG;
  int64_t blk = blockIdx.x;
  if (per_xcd > 0) blk = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  const int64_t c = blk * 4 + (threadIdx.x >> 6);
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const int sl = lane & (G - 1), gbase = lane & ~(G - 1);
  const int64_t row = chunk_row[c];
  const int64_t eb = chunk_ebase[c];
  const int64_t rb = rowptr[row];
  const int64_t rem = rowptr[row + 1] - eb;
  const int n = rem < 64 ? (int)rem : 64;
  const int my_e = CL::held_edge(lane, 0), my_e1 = CL::held_edge(lane, 1);
  const uint32_t cl = col[eb + (my_e < n ? my_e : 0)];
  uint32_t cl1 = 0;
  if constexpr (G == 32) cl1 = col[eb + (my_e1 < n ? my_e1 : 0)];
  const int head = sl / LH;
  using P4 = Pair4<E>;
  const uint32_t ldb = (uint32_t)(P4::DW * len + 4 * H) * 4u;   // bytes of a table row
  const uint32_t lane_off = (uint32_t)sl * P4::BYTES;           // this lane's (h0 g0 h1 g1 h2 g2 h3 g3)
  const uint32_t rec_off = (uint32_t)(P4::DW * len) * 4u + (uint32_t)head * 16u;
  const char* Tb = reinterpret_cast<const char*>(T);
  auto row_at = [&](uint32_t v, uint32_t off) { return *reinterpret_cast<const f4*>(Tb + (size_t)(v * ldb + off)); };
  const uint32_t ri = (uint32_t)row;
  f4 qi0, qi1;
  {
    f2 o0, o1, o2, o3;
    P4::widen(P4::load(Tb, ri * ldb + lane_off), o0, o1, o2, o3);
    qi0 = f4{o0[0], o0[1], o1[0], o1[1]};
    qi1 = f4{o2[0], o2[1], o3[0], o3[1]};
  }
  const f4 reci = row_at(ri, rec_off);
  const f4 al4 = *reinterpret_cast<const f4*>(alpha_l + sl * 4);
  const f4 ar4 = *reinterpret_cast<const f4*>(alpha_r + sl * 4);
  // loop-invariant left operands of the two chains: (grad_i[k], h_i[k]) and (a_r[k], a_l[k])
  const f2 GH[4] = {{qi0[1], qi0[0]}, {qi0[3], qi0[2]}, {qi1[1], qi1[0]}, {qi1[3], qi1[2]}};
  const f2 RL[4] = {{ar4[0], al4[0]}, {ar4[1], al4[1]}, {ar4[2], al4[2]}, {ar4[3], al4[3]}};
  // (sl_i, sr_i): the row's own dots, formed like the columns' below
  f2 SI;
  {
    float a = __builtin_fmaf(al4[3], qi1[2], __builtin_fmaf(al4[2], qi1[0], __builtin_fmaf(al4[1], qi0[2], al4[0] * qi0[0])));
    float b = __builtin_fmaf(ar4[3], qi1[2], __builtin_fmaf(ar4[2], qi1[0], __builtin_fmaf(ar4[1], qi0[2], ar4[0] * qi0[0])));
    float z0 = 0.f, z1 = 0.f;
    lanes_sum4_dpp<LH>(a, b, z0, z1);
    SI = f2{a, b};
  }
  const float rd_i = reci[0], m_i = reci[1], is_i = reci[2];
  const f2 eps2 = {eps, eps};
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  f2 S = {0.f, 0.f};  // (partial row sum of g, partial column sum of g)
#pragma unroll
  for (int j = 0; j < G; j += U) {
    if (j * NG >= n) break;  // (wave-uniform: no edge of the chunk is left for any group)
    typename P4::Raw q[U];
    f4 rc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t cj = (uint32_t)CL::step_value((int)cl, (int)cl1, lane, j + u);
      const uint32_t base = cj * ldb;
      q[u] = P4::load(Tb, base + lane_off);
      rc[u] = *reinterpret_cast<const f4*>(Tb + (size_t)(base + rec_off));
    }
    __builtin_amdgcn_sched_barrier(0);  // all loads of the batch are issued before the first one is consumed
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = CL::step_edge(lane, j + u) < n;
      f2 e0, e1, e2, e3;
      P4::widen(q[u], e0, e1, e2, e3);
      // P = (dpe, dpr) = (<grad_i, h_c>, <h_i, grad_c>)
      f2 P = GH[0] * e0;
      P = __builtin_elementwise_fma(GH[1], e1, P);
      P = __builtin_elementwise_fma(GH[2], e2, P);
      P = __builtin_elementwise_fma(GH[3], e3, P);
      // Q = (sr_c, sl_c) = (<a_r, h_c>, <a_l, h_c>)
      f2 Q = RL[0] * f2{e0[0], e0[0]};
      Q = __builtin_elementwise_fma(RL[1], f2{e1[0], e1[0]}, Q);
      Q = __builtin_elementwise_fma(RL[2], f2{e2[0], e2[0]}, Q);
      Q = __builtin_elementwise_fma(RL[3], f2{e3[0], e3[0]}, Q);
      float dpe = P[0], dpr = P[1], src = Q[0], slc = Q[1];
      lanes_sum4_dpp<LH>(dpe, dpr, src, slc);
      const f2 Tt = SI + f2{src, slc};  // pre-activation scores of (i -> c) and (c -> i)
      const f2 Tm = eps2 * Tt;
      const bool pe = Tt[0] > 0.0f, pr = Tt[1] > 0.0f;
      const float le = pe ? Tt[0] : Tm[0], lr = pr ? Tt[1] : Tm[1];
      const float a = __expf(le - m_i) * is_i;
      const float b = __expf(lr - rc[u][1]) * rc[u][2];
      // g = p (dp - rowdot) * leaky-relu'
      const f2 Gv = f2{a * (dpe - rd_i), b * (dpr - rc[u][0])} * f2{pe ? 1.0f : eps, pr ? 1.0f : eps};
      if (live) {  // (lanes past the end of a short chunk looked at the chunk's first edge: nothing of it is added)
        S += Gv;
        acc[0] = __builtin_fmaf(b, e0[1], acc[0]);
        acc[1] = __builtin_fmaf(b, e1[1], acc[1]);
        acc[2] = __builtin_fmaf(b, e2[1], acc[2]);
        acc[3] = __builtin_fmaf(b, e3[1], acc[3]);
      }
    }
  }
  float s_e = S[0], s_r = S[1];
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
    s_e += __shfl_xor(s_e, o, 64);
    s_r += __shfl_xor(s_r, o, 64);
  }
  const int64_t slot = (int64_t)chunk_start[row] + (eb - rb) / 64;
  if (gbase == 0) {
    *reinterpret_cast<f4*>(out_partial + slot * len + sl * 4) = acc;
    if ((sl & (LH - 1)) == 0) {
      rc_partial[slot * 2 * H + head] = s_e;      // partial row sum of g    (-> alpha_l gradient)
      rc_partial[slot * 2 * H + H + head] = s_r;  // partial column sum of g (-> alpha_r gradient)
    }
  }
}

// ---- forward in ONE sweep: scores, edge softmax and aggregation over the ordered chunk list ---------------------------
// GAT_Aggregator::aggregate (gat_aggregator.cpp:57-97) staged = per-vertex dots, a row-owner pass writing p [ne][H]
// (two sweeps over long rows), then the aggregation reading p.  Here a chunk's wave gathers the rows h_c once, forms
// sr_c = a_r . h_c from the gathered row, t = leaky_relu(sl_i + sr_c), and keeps an ONLINE softmax per lane group:
// running maximum m, running sum s of exp(t - m) and the running weighted row sum, rescaled by exp(m_old - m_new) when
// the maximum moves; the four groups and then the row's chunks are combined the same way (gat_fwd_reduce_kernel):
//   out_i = sum_c exp(m_c - M) acc_c / S,   S = sum_c exp(m_c - M) s_c,   M = max_c m_c
// which is the reference's max-subtracted softmax (math_functions.cpp:485-494) up to fp32 rounding.  Nothing per edge is
// written: backward forms p again from stats[v][h] = (M, 1/S) (gat_bwd_fused_chunk_kernel<RECOMP>).
constexpr float GAT_NEG = -1.0e30f;  // "no edge yet": finite, so exp(NEG - m) = 0 and NEG - NEG = 0 (not NaN)

// DROP: out_i = sum_e p_e w_e h_c with w = mask . scale (gat_drop_bits); (m, ssum) and so the row statistics are the
// undropped softmax's.  The three trailing arguments are the DROP form's.
// WIDE: feat has rows of ld elements of which this launch sweeps len = 4 G; the partials stay len wide.
// DROP && WIDE: the masks' index window (gat_drop_bits<.., WIN>) from the two arguments behind ld.
template <int G, int H, int U, typename E, bool DROP = false, bool WIDE = false>
__global__ __launch_bounds__(256) void gat_fwd_fused_chunk_kernel(
    int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase, const uint32_t* chunk_start,
    const int64_t* rowptr, const uint32_t* col, int len, const E* feat, const float* alpha_l, const float* alpha_r,
    float eps, float* out_partial, float2* ms_partial, int phase, uint32_t own_cols, int per_xcd, float drop_rate = 0.0f,
    float drop_scale = 1.0f, uint64_t drop_seed = 0, int ld = 0, int mask_heads = 0, int mask_head0 = 0) {
  const int fld = WIDE ? ld : len;  // row stride of feat
  constexpr int LH = G / H;
  using CL = ChunkLanes<G>;
  constexpr int NG = CL::NG;
  int64_t blk = blockIdx.x;  // (per_xcd: see gat_bwd_fused_chunk_kernel)
  if (per_xcd > 0) blk = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  const int64_t c = blk * 4 + (threadIdx.x >> 6);
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const int sl = lane & (G - 1), gbase = lane & ~(G - 1);
  const int64_t row = chunk_row[c];
  const int64_t eb = chunk_ebase[c];
  const int64_t rb = rowptr[row];
  const int64_t rem = rowptr[row + 1] - eb;
  const int n = rem < 64 ? (int)rem : 64;

  // step t of lane group g = edge t * NG + g; the column ids once, in DPP reach (ChunkLanes, see the backward kernel)
  const int my_e = CL::held_edge(lane, 0), my_e1 = CL::held_edge(lane, 1);
  const uint32_t cl = col[eb + (my_e < n ? my_e : 0)];
  uint32_t cl1 = 0;
  if constexpr (G == 32) cl1 = col[eb + (my_e1 < n ? my_e1 : 0)];
  if (phase >= 0 && ((__ballot((my_e < n && cl >= own_cols) || (G == 32 && my_e1 < n && cl1 >= own_cols)) == 0) != (phase == 0))) return;
  const int coff = sl * 4;
  const int head = sl / LH;
  using R4 = Row4<E>;
  const f4 hi = R4::widen(load_row4(feat + row * (int64_t)fld + coff));
  const f4 al4 = *reinterpret_cast<const f4*>(alpha_l + coff);
  const f4 ar4 = *reinterpret_cast<const f4*>(alpha_r + coff);
  auto d4 = [](const f4& a, const f4& b) {
    return __builtin_fmaf(a[3], b[3], __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0])));
  };
  const float sl_i = lanes_sum_w<LH>(d4(al4, hi));  // (DPP sums / broadcasts, FMA chains: see the backward kernel)
  uint32_t mb = 0;  // DROP: the masks of the chunk's edges, one bit per step (gat_drop_bits)
  if constexpr (DROP) mb = gat_drop_bits<G, H, false, WIDE>(lane, n, eb, nullptr, drop_seed, drop_rate, mask_heads, mask_head0);
  float m = GAT_NEG, ssum = 0.f;
  f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < G; j += U) {
    if (j * NG >= n) break;  // (wave-uniform)
    typename R4::Raw xh_raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t cj = (uint32_t)CL::step_value((int)cl, (int)cl1, lane, j + u);
      xh_raw[u] = load_row4(feat + (int64_t)cj * fld + coff);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const f4 xh = R4::widen(xh_raw[u]);
      const float sr_c = lanes_sum_w<LH>(d4(ar4, xh));
      if (CL::step_edge(lane, j + u) < n) {  // uniform per group; lanes past the end of a short chunk add nothing
        const float t0 = sl_i + sr_c;
        const float t = t0 > 0.0f ? t0 : eps * t0;
        // online softmax: one of exp(m - max), exp(t - max) is exp(0) -- ONE exponential per edge
        const float d = t - m;
        const float ex = __expf(d > 0.f ? -d : d);
        const float sc = d > 0.f ? ex : 1.f, e = d > 0.f ? 1.f : ex;
        ssum = __builtin_fmaf(ssum, sc, e);
        if constexpr (DROP) {  // the softmax (m, ssum) does not see the mask; the aggregated term does
          const float ew = e * (((mb >> (j + u)) & 1u) ? drop_scale : 0.0f);
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(ew, xh[k], acc[k] * sc);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(e, xh[k], acc[k] * sc);
        }
        m = d > 0.f ? t : m;
      }
    }
  }
  // the four groups meet: same rescaling
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
    const float mo = __shfl_xor(m, o, 64), so = __shfl_xor(ssum, o, 64);
    const float mn = mo > m ? mo : m;
    const float a = expf(m - mn), b = expf(mo - mn);
    ssum = ssum * a + so * b;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = acc[k] * a + __shfl_xor(acc[k], o, 64) * b;
    m = mn;
  }
  const int64_t slot = (int64_t)chunk_start[row] + (eb - rb) / 64;
  if (gbase == 0) {
    *reinterpret_cast<f4*>(out_partial + slot * len + coff) = acc;
    if ((sl & (LH - 1)) == 0) ms_partial[slot * H + head] = float2{m, ssum};
  }
}

// per row: combine the chunks' (m, s, acc) in chunk order; out = act(sum / S); stats[row][h] = (M, 1/S)
// (a row is G = len / 4 lanes of 4 columns, so the wave's NG = 64 / G lane groups take the row's chunks k, k + 1, ...,
// k + NG - 1, ... and meet at the end -- at len 64 a row with 330 chunks is 83 steps deep instead of 330, and no lane idles)
// WIDE: out has rows of ld floats and stats rows of stats_ld records (a window of H heads in each); the partials are len / H wide
template <int G, bool WIDE = false>
__global__ __launch_bounds__(256) void gat_fwd_reduce_kernel(int64_t nv, int len, int H, const uint32_t* chunk_start,
                                                             const float* out_partial, const float2* ms_partial, int relu,
                                                             float* out, float2* stats, int ld = 0, int stats_ld = 0) {
  const int out_ld = WIDE ? ld : len, sld = WIDE ? stats_ld : H;
  constexpr int NG = 64 / G;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const int sl = lane & (G - 1), grp = lane / G;
  const int64_t c0 = chunk_start[row], c1 = chunk_start[row + 1];
  const int dh = len / H, head = (sl * 4) / dh;
  float M = GAT_NEG;
  for (int64_t k = c0 + grp; k < c1; k += NG) {
    const float mk = ms_partial[k * H + head].x;
    M = mk > M ? mk : M;
  }
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
    const float mo = __shfl_xor(M, o, 64);
    M = mo > M ? mo : M;
  }
  float S = 0.f;
  f4 s = {0.f, 0.f, 0.f, 0.f};
  for (int64_t k = c0 + grp; k < c1; k += NG) {
    const float2 ms = ms_partial[k * H + head];
    const float w = __expf(ms.x - M);
    S += ms.y * w;
    const f4 t = *reinterpret_cast<const f4*>(out_partial + k * len + sl * 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += t[q] * w;
  }
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {  // fixed order: deterministic
    S += __shfl_xor(S, o, 64);
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += __shfl_xor(s[q], o, 64);
  }
  if (grp != 0) return;
  const float inv = S > 0.f ? 1.0f / S : 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    s[q] *= inv;
    if (relu) s[q] = s[q] > 0.f ? s[q] : 0.f;
  }
  *reinterpret_cast<f4*>(out + row * (int64_t)out_ld + sl * 4) = s;
  if ((sl * 4) % dh == 0) stats[row * sld + head] = float2{M, inv};
}

// out[row] = sum of the row's chunk partials in chunk order; rs / cs [row][H] the same for the g sums
// WIDE: out has rows of ld floats; the partials, rs and cs are the slab's own
template <int G, bool WIDE = false>
__global__ __launch_bounds__(256) void gat_fused_reduce_kernel(int64_t nv, int len, int H, const uint32_t* chunk_start,
                                                               const float* out_partial, const float* rc_partial,
                                                               float* out, float* rs, float* cs, int ld = 0) {
  const int out_ld = WIDE ? ld : len;
  constexpr int NG = 64 / G;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const int sl = lane & (G - 1), grp = lane / G;  // NG lane groups share the row's chunks (see the forward's)
  const int64_t c0 = chunk_start[row], c1 = chunk_start[row + 1];
  f4 s = {0.f, 0.f, 0.f, 0.f};
  // this lane's share of the 2 H row / column sums: entries sl, sl + G, sl + 2 G, sl + 3 G (2 H <= 32, G >= 8)
  float r[4] = {0.f, 0.f, 0.f, 0.f};
  const float* pp = out_partial + sl * 4;
  for (int64_t k = c0 + grp; k < c1; k += NG) {
    const f4 t = *reinterpret_cast<const f4*>(pp + k * len);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (sl + q * G < 2 * H) r[q] += rc_partial[k * 2 * H + sl + q * G];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += t[q];
  }
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {  // fixed order: deterministic
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] += __shfl_xor(r[q], o, 64);
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += __shfl_xor(s[q], o, 64);
  }
  if (grp != 0) return;
  *reinterpret_cast<f4*>(out + row * (int64_t)out_ld + sl * 4) = s;
  // entries 0..H-1: rs, H..2H-1: cs
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = sl + q * G;
    if (e < H) rs[row * H + e] = r[q];
    else if (e < 2 * H) cs[row * H + e - H] = r[q];
  }
}

inline unsigned rowgrid(int64_t nv) { return (unsigned)cdiv64(nv > 0 ? nv : 1, 4); }

}  // namespace

// the one-sweep kernels' shapes (round 5): len = 32, 64 or 128 (8, 16 or 32 lanes x 4 columns per edge) and 1, 2, 4, 8 or 16
// heads with at least 4 columns per head -- every head width the reference's GAT runs up to its limit of 128 columns
// (gat_aggregator.cpp:57-200, global.h:58) as long as a head is a whole number of 4-column lanes
static bool gat_fused_shape(int len, int heads) {
  if (!(len == 32 || len == 64 || len == 128)) return false;
  if (!(heads == 1 || heads == 2 || heads == 4 || heads == 8 || heads == 16)) return false;
  return heads * 4 <= len;
}
// M(G, H) for the kernel instance of a shape gat_fused_shape() admits
#define GAIB_GAT_BY_HEADS(G, M, WITH16) \
  switch (heads) {                      \
    case 1: M(G, 1); break;             \
    case 2: M(G, 2); break;             \
    case 4: M(G, 4); break;             \
    case 8: M(G, 8); break;             \
    default: WITH16; break;             \
  }
#define GAIB_GAT_DISPATCH(M)                                    \
  do {                                                          \
    if (len == 32) { GAIB_GAT_BY_HEADS(8, M, (void)0) }         \
    else if (len == 64) { GAIB_GAT_BY_HEADS(16, M, M(16, 16)) } \
    else { GAIB_GAT_BY_HEADS(32, M, M(32, 16)) }                \
  } while (0)

static size_t up4(size_t n) { return (n + 3) & ~(size_t)3; }  // keep every part of a workspace 16-byte aligned

static int check_heads(const char* who, int len, int heads) {
  GAIB_CHECK(len > 0, "%s: len must be > 0", who);
  GAIB_CHECK(heads >= 1 && len % heads == 0, "%s: heads (%d) must divide len (%d)", who, heads, len);
  return GAIB_OK;
}

// the packed-math sweep for the shapes it covers (a head of at most 16 lanes); the others never get here (see `pk` below)
template <int G, int H, typename E>
static void launch_bwd_pk(unsigned grid, hipStream_t st, int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase,
                          const uint32_t* chunk_start, const int64_t* rowptr, const uint32_t* col, int len, const E* T,
                          const float* alpha_l, const float* alpha_r, float eps, float* out_partial, float* rc_partial, int per_xcd) {
  if constexpr (G / H <= 16) {
    gat_bwd_fused_pk_kernel<G, H, 4, E><<<grid, 256, 0, st>>>(n_chunks, chunk_row, chunk_ebase, chunk_start, rowptr, col, len, T, alpha_l,
                                                          alpha_r, eps, out_partial, rc_partial, per_xcd);
  }
}

// The fused edge side of backward (gat_bwd_fused_chunk_kernel).  Shapes: gat_fused_shape(); otherwise, or with the option off (option
// gat_fused_bwd: 0 = never; -1 / 1 = whenever the shape fits), GAIB_ERR_UNSUPPORTED is returned and nothing was touched: the
// caller runs the staged entry points.
static bool gat_fused_applies(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int knob, uintptr_t align_or, int* rc,
                              bool rect = false) {
  *rc = GAIB_OK;
  // On a rank's rectangular graph the answer must follow from rank-INVARIANT inputs alone -- len, heads, the option:
  // the one-sweep and the staged path run different collectives in backward, so a rank that has rows but no edges (an
  // empty sweep is a valid sweep) or a misaligned buffer must not take another path than its peers (the latter is an
  // error, not a reason to fall back).
  const bool heads_ok = gat_fused_shape(len, heads);
  if (rect) {
    if (heads_ok && knob != 0 && (align_or & 15) != 0) {
      gaib_set_error("one-sweep GAT on a partition: buffers must be 16-byte aligned");
      *rc = GAIB_ERR_INVALID;
      return false;
    }
    return heads_ok && knob != 0;
  }
  // Round 5: the rule is the SHAPE.  Until round 4 the automatic choice (knob < 0) also asked for a dense graph (a quarter of
  // the edges in heavy rows) over a table of <= 512 MB -- the rule of the ordered-chunk aggregation.  Measured with the kernels
  // at every width (scripts/perf_guard.py, profiles/r05/perf_guard.log): the one sweep wins wherever it applies -- reddit shape
  // 8 heads x 32: 5.06 vs 15.95 ms per layer step, x 64: 8.8 vs 17.8, x 128: 18.4 vs 26.0; products shape (sparse: one short
  // chunk per row, a 627 MB table) 1 head x 64: 19.7 vs 21.2 -- so nothing is left for the staged kernels but the widths
  // outside gat_fused_shape(), attention dropout and the explicit option.
  const bool shape_ok = heads_ok && g->nc == g->nv && g->ne > 0 && (align_or & 15) == 0;
  return shape_ok && knob != 0;
}

// alpha_l' = sum_v rs[v] x[v], alpha_r' = sum_v cs[v] x[v]: partial sums over gat_alpha_blocks(nv) strips of rows (partial:
// [blocks][2][len] floats), then one wave per output element.  WIDE: x has rows of ld elements.
static int gat_alpha_blocks(int64_t nv) { return (int)(nv < 2048 ? cdiv64(nv, 8) : 1024); }
template <typename E, bool WIDE = false>
static int launch_alpha_grads(gaib_ctx* ctx, int64_t nv, int len, int heads, const E* d_x, const float* rs, const float* cs,
                              float* partial, float* d_alpha_lgrad, float* d_alpha_rgrad, int ld = 0) {
  const int nblocks = gat_alpha_blocks(nv);
  alpha_partial_kernel<E, WIDE><<<nblocks, 256, sizeof(float) * 512, ctx->stream>>>(nv, len, heads, d_x, rs, cs, cdiv64(nv, nblocks),
                                                                                  partial, ld);
  GAIB_LAUNCH_CHECK();
  alpha_final_kernel<<<(unsigned)cdiv64(2 * (int64_t)len, 4), 256, 0, ctx->stream>>>(nblocks, len, partial, d_alpha_lgrad, d_alpha_rgrad);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}
