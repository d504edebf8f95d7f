// gatv2_kernels.h -- the one-sweep GATv2 (dynamic attention, Brody / Alon / Yahav): the score moves the leaky relu INSIDE the dot
// product,
//   s_ij^k = sum_{c in C_k} a_c phi(h_ic + h_jc),     phi(x) = x > 0 ? x : eps x
// with ONE shared vector a, so s_ij = s_ji.  gatv2.hip (fp32 tables) and gatv2_bf16.hip (bf16 tables) instantiate the two sweeps
// through the host sequences of gatv2_seq.h; the chunk list,
// the XCD walk, ChunkLanes<G>, rowdot_kernel, gat_rec_kernel and the chunk-order row reductions are gat_kernels.h's, unchanged.
//
// Lanes (gat_fused_shape): a row is G = len / 4 lanes of 4 columns (one gather per lane and edge: 16 bytes of fp32, 8 of bf16), a wave works on
// NG = 64 / G edges per step, head k owns LH = G / H consecutive lanes.  The score needs no gathered byte the aggregation does not
// gather anyway: the row h_j is in registers when its score is formed.
//
// THE ORDER OF A SCORE'S SUM (gatv2_score, the one place it is written): per lane z_q = h_i[q] + h_j[q] for its columns
// q = 0..3, t = a_0 phi(z_0), then t = fma(a_q, phi(z_q), t) for q = 1, 2, 3 (ascending columns); then the butterfly over the head's
// lanes, partner lane ^ 1, ^ 2, ^ 4, ^ 8 (DPP inside the 16-lane row) and ^ 16 (LH = 32).  z is commutative bit for bit, the
// chain does not know which operand was the row's own, and both sides of a butterfly stage add the same two values: every lane
// of the head holds the same bits, and they are the bits of s_ij in the forward sweep, of s_ij in the backward sweep and of s_ji
// in the chunk of row i.  The backward sweep RESTS on that: it forms p_ij = exp(s_ij - m_i) / l_i from the statistics of the
// OTHER end i, and only because s_ij is bit for bit one of the scores row i's forward sweep took its maximum m_i over is the
// exponent never positive, whatever the size of the scores.
#pragma once
#include "gat_kernels.h"

namespace {

// phi per column, and the score of the edge between the rows hi (the chunk's own) and xh (gathered); pz: phi(z) for the caller
template <int LH>
__device__ __forceinline__ float gatv2_score(const f4& a4, const f4& hi, const f4& xh, float eps, f4& z, f4& pz) {
  z = hi + xh;
  const f4 ze = z * eps;
#pragma unroll
  for (int q = 0; q < 4; ++q) pz[q] = z[q] > 0.0f ? z[q] : ze[q];
  const float t = __builtin_fmaf(a4[3], pz[3], __builtin_fmaf(a4[2], pz[2], __builtin_fmaf(a4[1], pz[1], a4[0] * pz[0])));
  return lanes_sum_w<LH>(t);
}

// a lane's four columns of row v AS LOADED (Row4<E>::Raw: 16 bytes of fp32, 8 bytes of raw bf16 bits) from a table whose fp32 form is
// below 4 GB: one 32-bit byte offset per edge (a VALU multiply instead of a 64-bit chain).  The 16-byte records are E = float
template <typename E>
__device__ __forceinline__ typename Row4<E>::Raw gatv2_row4(const char* tab, uint32_t v, uint32_t row_bytes, uint32_t lane_off) {
  return load_row4(reinterpret_cast<const E*>(tab + (size_t)(v * row_bytes + lane_off)));
}

// ---- forward: scores, ONLINE softmax and aggregation of a 64-edge chunk --------------------------------------------------------
// Per batch of U steps a lane group gathers U rows, forms their U scores, takes the maximum over the batch and its running
// maximum FIRST and rescales (m, l, acc) once per batch, not per edge: U + 1 exponentials and one rescale of the accumulator per
// U edges.  The NG groups and then the row's chunks meet by the same rule; the partials (m, l) [slot][H] and acc [slot][len] have
// gat_fwd_fused_chunk_kernel's format, so gat_fwd_reduce_kernel merges them in chunk order and writes out and row_stats.
// Nothing per edge is written.
// WIDE: feat has rows of ld floats of which this launch sweeps the len = 4 G at `feat` (one column slab of a wider multi-head row,
// option gatv2_wide); a is the slab's piece and the partials stay len wide.  A template flag with a trailing, defaulted argument read
// only behind `WIDE ? ld : len`: the narrow instantiations compile to the instructions they had.
// DROP: attention dropout inside the sweep, out_i = act(sum_j p_ij w_ij h_j) with w = mask . scale of element e heads + k of the
// [ne][heads] array gaib_dropout fills (gat_drop_bits: one bit word per chunk, formed ahead of the edge loop; under WIDE the slab's
// head window mask_heads / mask_head0 of the full row).  The softmax does not see the mask: the maximum, l and so the row
// statistics are the undropped sweep's; only the accumulator's weight e becomes e w, a bit test and a select.  The five trailing
// arguments are read behind the flag only.
// E: the element type of feat (float; uint16_t = raw bf16 bits, gatv2_bf16.hip).  The chunk's own row is widened once, a gathered
// row waits as loaded and is widened (Row4<E>::widen: exact, the identity for float) on the consume side of the batch's
// sched_barrier; everything behind the widening is one text, so the bf16 sweep has the bits of the fp32 sweep on the widened table.
template <int G, int H, int U, bool WIDE = false, bool DROP = false, typename E = float>
__global__ __launch_bounds__(256) void gatv2_fwd_chunk_kernel(int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase,
                                                              const uint32_t* chunk_start, const int64_t* rowptr, const uint32_t* col,
                                                              const E* feat, const float* a, float eps, float* out_partial,
                                                              float2* ms_partial, int per_xcd, int ld = 0, float drop_rate = 0.0f,
                                                              float drop_scale = 1.0f, uint64_t drop_seed = 0, int mask_heads = 0,
                                                              int mask_head0 = 0) {
  constexpr int LH = G / H, len = 4 * G;
  using CL = ChunkLanes<G>;
  using R4 = Row4<E>;
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
  const int my_e = CL::held_edge(lane, 0), my_e1 = CL::held_edge(lane, 1);
  const uint32_t cl = col[eb + (my_e < n ? my_e : 0)];
  uint32_t cl1 = 0;
  if constexpr (G == 32) cl1 = col[eb + (my_e1 < n ? my_e1 : 0)];
  const int coff = sl * 4, head = sl / LH;
  const char* tab = reinterpret_cast<const char*>(feat);
  // (WIDE: the FULL row's bytes -- v * row_bytes + lane_off is below nv * ld * 4, which the host holds under 4 GB)
  const uint32_t row_bytes = (uint32_t)(WIDE ? ld : len) * (uint32_t)sizeof(E), lane_off = (uint32_t)coff * (uint32_t)sizeof(E);
  const f4 hi = R4::widen(gatv2_row4<E>(tab, (uint32_t)row, row_bytes, lane_off));
  const f4 a4 = *reinterpret_cast<const f4*>(a + coff);
  uint32_t mb = 0;  // DROP: the masks of the chunk's edges for this lane's head, bit t = step t
  if constexpr (DROP) mb = gat_drop_bits<G, H, false, WIDE>(lane, n, eb, nullptr, drop_seed, drop_rate, mask_heads, mask_head0);
  float m = GAT_NEG, l = 0.f;
  f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < G; j += U) {
    if (j * NG >= n) break;  // (wave-uniform)
    typename R4::Raw xr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) xr[u] = gatv2_row4<E>(tab, (uint32_t)CL::step_value((int)cl, (int)cl1, lane, j + u), row_bytes, lane_off);
    __builtin_amdgcn_sched_barrier(0);  // all gathers of the batch are issued before the first one is consumed
    float s[U], mx = m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      f4 z, pz;
      s[u] = gatv2_score<LH>(a4, hi, R4::widen(xr[u]), eps, z, pz);
      // (lanes past the end of a short chunk looked at the chunk's first edge: its score takes no part)
      if (CL::step_edge(lane, j + u) < n) mx = s[u] > mx ? s[u] : mx;
    }
    const float sc = __expf(m - mx);  // (no edge yet on either side: NEG - NEG = 0 and the empty sums stay 0)
    l *= sc;
    acc *= sc;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float e = CL::step_edge(lane, j + u) < n ? __expf(s[u] - mx) : 0.0f;
      l += e;  // (undropped under DROP too)
      float ew = e;
      if constexpr (DROP) ew = e * (((mb >> (j + u)) & 1u) ? drop_scale : 0.0f);
      const f4 xh = R4::widen(xr[u]);  // (bf16: widened a second time, two VALU per column, not kept across the batch's maximum)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __builtin_fmaf(ew, xh[q], acc[q]);
    }
    m = mx;
  }
  // the NG groups meet: the same rescaling, in a fixed order
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
    const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
    const float mn = mo > m ? mo : m;
    const float wa = expf(m - mn), wb = expf(mo - mn);
    l = l * wa + lo * wb;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = acc[q] * wa + __shfl_xor(acc[q], o, 64) * wb;
    m = mn;
  }
  const int64_t slot = (int64_t)chunk_start[row] + (eb - rb) / 64;
  if (gbase == 0) {
    *reinterpret_cast<f4*>(out_partial + slot * len + coff) = acc;
    if ((sl & (LH - 1)) == 0) ms_partial[slot * H + head] = float2{m, l};
  }
}

// ---- backward: the whole input gradient and a's gradient in ONE sweep over the chunks of row j ------------------------------------
// With s_ij = s_ji and a structurally symmetric graph, the in-edges of j are the reverses of its own edges, so row j's chunk sees
// both ends of the attention-score path of every edge {i, j} it holds:
//   p_ij = exp(s - m_i) / l_i    dp_ij = <g_i, h_j>    ds_ij = p_ij (dp_ij - delta_i)      i attends to j: i's record, gathered
//   p_ji = exp(s - m_j) / l_j    dp_ji = <g_j, h_i>    ds_ji = p_ji (dp_ji - delta_j)      j attends to i: j's own registers
//   grad_out_j += p_ij g_i + (ds_ij + ds_ji) a phi'(h_i + h_j)
//   a_grad     += ds_ji phi(h_j + h_i)                                                     (each directed edge once, in its row)
// Per edge: the rows h_i and g_i and the 16-byte record (delta_i, m_i, 1 / l_i) of the head -- what the v1 sweep gathers -- and
// three sums over the head's lanes (s and the two dot products).  grad_out leaves as one partial row per chunk, summed per row in
// chunk order (gat_fused_reduce_kernel); a's gradient lives in four registers per lane across the chunk, meets over the lane
// groups and the workgroup's four waves in a fixed order and leaves as ONE partial vector per workgroup (agrad_partial
// [gridDim.x][len], summed by gatv2_agrad_strip_kernel / gatv2_agrad_final_kernel).  No atomics, nothing per edge is written.
// WIDE: feat and grad have rows of ld floats (see the forward); the records [nv][H] and both partials are the slab's own.
// DROP: the forward was out_i = act(sum_j p_ij w_ij h_j).  delta_i = <g_i, out_i> with the DROPPED output is still sum_j p_ij dp_ij,
// so the records are unchanged, and
//   dp_ij = w_ij <g_i, h_j>      dp_ji = w_ji <g_j, h_i>      grad_out_j += p_ij w_ij g_i + (ds_ij + ds_ji) a phi'(h_i + h_j)
// -- a dropped edge still enters ds through -p delta.  The two directions of an edge carry DIFFERENT masks while the score stays
// symmetric bit for bit, so the one sweep still suffices: row j's chunk holds e = e(j -> i), w_ji is element e heads + k (the row
// side of gat_drop_bits, whose key advances by addition) and w_ij element rev[e] heads + k (rev read at the lane's own steps, 256
// contiguous bytes per chunk).  Two bit words per chunk, formed ahead of the edge loop; in the loop two bit tests and selects.
// The six trailing arguments are read behind the flag only.
// E: the element type of feat and grad, as in the forward: h_j and g_j are widened once per chunk, the gathered h_i and g_i wait as
// loaded (bf16: 2 + 2 + 4 registers per edge in flight instead of 4 + 4 + 4) and are widened behind the sched_barrier.
template <int G, int H, int U, bool WIDE = false, bool DROP = false, typename E = float>
__global__ __launch_bounds__(256) void gatv2_bwd_chunk_kernel(int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase,
                                                              const uint32_t* chunk_start, const int64_t* rowptr, const uint32_t* col,
                                                              const E* feat, const E* grad, const f4* rec, const float* a,
                                                              float eps, float* out_partial, float* agrad_partial, int per_xcd,
                                                              int ld = 0, const uint32_t* rev = nullptr, float drop_rate = 0.0f,
                                                              float drop_scale = 1.0f, uint64_t drop_seed = 0, int mask_heads = 0,
                                                              int mask_head0 = 0) {
  constexpr int LH = G / H, len = 4 * G;
  using CL = ChunkLanes<G>;
  using R4 = Row4<E>;
  constexpr int NG = CL::NG;
  __shared__ float sm[4 * len];
  int64_t blk = blockIdx.x;
  if (per_xcd > 0) blk = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  const int wv = threadIdx.x >> 6;
  const int64_t c = blk * 4 + wv;
  const int lane = threadIdx.x & 63;
  const int sl = lane & (G - 1), gbase = lane & ~(G - 1);
  const int coff = sl * 4, head = sl / LH;
  f4 ag = {0.f, 0.f, 0.f, 0.f};
  if (c < n_chunks) {  // (no early return: the workgroup meets below)
    const int64_t row = chunk_row[c];
    const int64_t eb = chunk_ebase[c];
    const int64_t rb = rowptr[row];
    const int64_t rem = rowptr[row + 1] - eb;
    const int n = rem < 64 ? (int)rem : 64;
    const int my_e = CL::held_edge(lane, 0), my_e1 = CL::held_edge(lane, 1);
    const uint32_t cl = col[eb + (my_e < n ? my_e : 0)];
    uint32_t cl1 = 0;
    if constexpr (G == 32) cl1 = col[eb + (my_e1 < n ? my_e1 : 0)];
    const char* ftab = reinterpret_cast<const char*>(feat);
    const char* gtab = reinterpret_cast<const char*>(grad);
    const char* rtab = reinterpret_cast<const char*>(rec);
    const uint32_t row_bytes = (uint32_t)(WIDE ? ld : len) * (uint32_t)sizeof(E), lane_off = (uint32_t)coff * (uint32_t)sizeof(E);
    const uint32_t rec_bytes = (uint32_t)H * 16u, rec_off = (uint32_t)head * 16u;
    const f4 hi = R4::widen(gatv2_row4<E>(ftab, (uint32_t)row, row_bytes, lane_off));
    const f4 gi = R4::widen(gatv2_row4<E>(gtab, (uint32_t)row, row_bytes, lane_off));
    const f4 ri = gatv2_row4<float>(rtab, (uint32_t)row, rec_bytes, rec_off);  // (delta_j, m_j, 1 / l_j)
    const f4 a4 = *reinterpret_cast<const f4*>(a + coff);
    const f4 ae4 = a4 * eps;  // a phi' where z <= 0
    uint32_t mb_e = 0, mb_r = 0;  // DROP: the masks of the chunk's edges (w_ji) and of their reverse edges (w_ij), bit t = step t
    if constexpr (DROP) {
      mb_e = gat_drop_bits<G, H, false, WIDE>(lane, n, eb, nullptr, drop_seed, drop_rate, mask_heads, mask_head0);
      mb_r = gat_drop_bits<G, H, true, WIDE>(lane, n, eb, rev, drop_seed, drop_rate, mask_heads, mask_head0);
    }
    auto d4 = [](const f4& x, const f4& y) {
      return __builtin_fmaf(x[3], y[3], __builtin_fmaf(x[2], y[2], __builtin_fmaf(x[1], y[1], x[0] * y[0])));
    };
    f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < G; j += U) {
      if (j * NG >= n) break;  // (wave-uniform)
      typename R4::Raw xh_raw[U], xg_raw[U];
      f4 rc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t cj = (uint32_t)CL::step_value((int)cl, (int)cl1, lane, j + u);
        xh_raw[u] = gatv2_row4<E>(ftab, cj, row_bytes, lane_off);
        xg_raw[u] = gatv2_row4<E>(gtab, cj, row_bytes, lane_off);
        rc[u] = gatv2_row4<float>(rtab, cj, rec_bytes, rec_off);
      }
      __builtin_amdgcn_sched_barrier(0);  // all gathers of the batch are issued before the first one is consumed
#pragma unroll
      for (int u = 0; u < U; ++u) {
        f4 z, pz;
        const f4 xh = R4::widen(xh_raw[u]), xg = R4::widen(xg_raw[u]);
        const float s = gatv2_score<LH>(a4, hi, xh, eps, z, pz);  // the forward's bits, from either end
        float dp_ji = lanes_sum_w<LH>(d4(gi, xh));
        float dp_ij = lanes_sum_w<LH>(d4(xg, hi));
        float w_ij = 1.0f;
        if constexpr (DROP) {  // (the sums are scaled after they met: with rate 0 and scale 1 the undropped bits)
          dp_ji *= ((mb_e >> (j + u)) & 1u) ? drop_scale : 0.0f;
          w_ij = ((mb_r >> (j + u)) & 1u) ? drop_scale : 0.0f;
          dp_ij *= w_ij;
        }
        const float p_ji = __expf(s - ri[1]) * ri[2];
        const float p_ij = __expf(s - rc[u][1]) * rc[u][2];
        const float ds_ji = p_ji * (dp_ji - ri[0]);
        const float ds_ij = p_ij * (dp_ij - rc[u][0]);
        const float ds = ds_ij + ds_ji;
        float pw_ij = p_ij;  // the gradient flows back along the DROPPED attention p_ij w_ij
        if constexpr (DROP) pw_ij = p_ij * w_ij;
        if (CL::step_edge(lane, j + u) < n) {  // (lanes past the end of a short chunk looked at its first edge: nothing is added)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            acc[q] = __builtin_fmaf(pw_ij, xg[q], acc[q]);
            acc[q] = __builtin_fmaf(ds, z[q] > 0.0f ? a4[q] : ae4[q], acc[q]);
            ag[q] = __builtin_fmaf(ds_ji, pz[q], ag[q]);
          }
        }
      }
    }
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {  // the NG groups meet, fixed order
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[q] += __shfl_xor(acc[q], o, 64);
        ag[q] += __shfl_xor(ag[q], o, 64);
      }
    }
    const int64_t slot = (int64_t)chunk_start[row] + (eb - rb) / 64;
    if (gbase == 0) *reinterpret_cast<f4*>(out_partial + slot * len + coff) = acc;
  }
  // the workgroup's four chunks meet in wave order (a wave without a chunk brings zeros)
  if (gbase == 0) *reinterpret_cast<f4*>(sm + wv * len + coff) = ag;
  __syncthreads();
  if (threadIdx.x < len) {
    const int t = threadIdx.x;
    // DROP: the vector is stored at the index of the workgroup's CHUNKS, so a's sum does not depend on the per_xcd walk (gatv2_seq.h)
    const int64_t slot_ag = DROP ? blk : (int64_t)blockIdx.x;
    agrad_partial[slot_ag * len + t] = ((sm[t] + sm[len + t]) + sm[2 * len + t]) + sm[3 * len + t];
  }
}

// strip[b][c] = sum of partial[v][c] over the rows v of strip b, rows_per_block each: thread t owns column t % len of every
// (256 / len)-th row, the 256 / len sub-sums meet in LDS in a fixed order (the pattern of alpha_partial_kernel).  One head of 256 or
// 512 columns: column passes of 256, thread t owns column pass * 256 + t of EVERY row of the strip, in row order
__global__ __launch_bounds__(256) void gatv2_agrad_strip_kernel(int64_t n, int len, const float* partial, int64_t rows_per_block,
                                                                float* strip) {
  __shared__ float sm[256];
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  if (len > 128) {  // (uniform over the grid: no thread of it reaches the barrier below)
    for (int c = threadIdx.x; c < len; c += 256) {
      float s = 0.f;
      for (int64_t v = r0; v < r1; ++v) s += partial[v * len + c];
      strip[(int64_t)blockIdx.x * len + c] = s;
    }
    return;
  }
  const int rpp = 256 / len, tc = threadIdx.x % len, tr = threadIdx.x / len;  // (len <= 128: at least two rows per pass)
  float s = 0.f;
  for (int64_t v = r0 + tr; v < r1; v += rpp) s += partial[v * len + tc];
  sm[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < len) {
    float t = 0.f;
    for (int k = 0; k < rpp; ++k) t += sm[k * len + threadIdx.x];
    strip[(int64_t)blockIdx.x * len + threadIdx.x] = t;
  }
}

// a_grad[c] = sum over the strips: one wave per column, lanes stride over the strips, then the fixed-order wave sum
__global__ __launch_bounds__(256) void gatv2_agrad_final_kernel(int nstrips, int len, const float* strip, float* a_grad) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= len) return;
  const int lane = threadIdx.x & 63;
  float s = 0.f;
  for (int b = lane; b < nstrips; b += 64) s += strip[(int64_t)b * len + w];
  s = wave_sum(s);
  if (lane == 0) a_grad[w] = s;
}

}  // namespace
