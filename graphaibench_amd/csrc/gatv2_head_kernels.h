// gatv2_head_kernels.h -- the one-sweep GATv2 for ONE head of 256 or 512 columns (option gatv2_wide; gatv2_head.hip instantiates
// these kernels, gatv2_seq.h holds the host sequence).  Column slabs cannot cut a head: s_ij = sum_c a_c phi(h_ic + h_jc) runs over the
// whole of it.  The layout is gat_head_kernels.h's, and its pieces are used as they are: one wave per 64-edge chunk, four chunks per
// workgroup, the per_xcd walk (head_chunk); a lane owns CPL = len / 64 columns as Q = CPL / 4 pieces of 16 bytes at columns
// q 256 + 4 lane (HeadRow, head_load); the chunk's ids are fetched once and handed out with readlane, so a row's base address is
// scalar arithmetic; the other vertex's record (delta, m, 1 / l) is one wave-uniform 16-byte load; U edges in flight with all loads
// of a batch ahead of a sched_barrier, and the steps past the end of a short chunk read the chunk's first edge and are skipped at
// the point of use.  A sum over the head is a sum over the wave: head_sum4, four values per call.
//
// THE ORDER OF A SCORE'S SUM (gatv2_head_score, the one place it is written, used by both sweeps): per lane z = x + y for its
// columns, then ONE FMA chain t = a_0 phi(z_0), t = fma(a_c, phi(z_c), t) through the pieces q = 0 .. Q - 1 and the four columns of
// each, ascending; then head_sum4's six DPP stages, which add lane to lane by lane number alone and treat their four operands
// alike, so the slot a score travels in does not matter.  z is commutative bit for bit and neither step knows which operand was the
// chunk's own row: s_ij has the same bits in the forward sweep, in row j's backward chunk and in row i's.  The backward sweep rests
// on that as the narrow one does (gatv2_kernels.h): it forms p_ij = exp(s_ij - m_i) / l_i from the statistics of the OTHER end, and
// m_i is the fp32 maximum over scores of which s_ij is, bit for bit, one -- the exponent is never positive.
// Scores are fp32: at |s| up to 50 the sum of 512 terms lies within a few 1e-6 of fp64, a relative error of that size in p, far
// inside the 1e-4 the outputs are held to (the static-score head sweep took fp64 for scores of +-100 on rows that underflow).
// Deterministic, no atomics; every store is a plain vector store.
#pragma once
#include "gat_head_kernels.h"

// gatv2_head.hip: the sweeps for ONE head of 256 or 512 columns (cpl = gaib_gat_fused_head_cpl; gatv2_head_kernels.h) with their
// per-row reductions.  forward: d_out and d_row_stats [nv][1][2]; backward: d_grad_out and the workgroups' partial vectors of a's
// gradient, agrad_partial [grid][len], for gatv2_agrad_strip_kernel.  drop: NULL, or rate, scale and seed of the call (its window
// fields are not read: one head); backward under dropout reads g->rev.  E: the element type of the tables h, feat and grad (float,
// uint16_t = raw bf16 bits: both instantiated in gatv2_head.hip and nowhere else)
template <typename E>
int gatv2_head_forward_run(gaib_ctx* ctx, const gaib_graph* g, int cpl, unsigned grid, int per_xcd, const E* h, const float* a,
                           float eps, int relu, float* out_partial, float2* ms_partial, float* out, float* row_stats,
                           const DropWin* drop);
template <typename E>
int gatv2_head_backward_run(gaib_ctx* ctx, const gaib_graph* g, int cpl, unsigned grid, int per_xcd, const E* feat, const E* grad,
                            const f4* rec, const float* a, float eps, float* out_partial, float* agrad_partial, float* grad_out,
                            const DropWin* drop);

namespace {

// this lane's part of the score of the edge between the rows x and y (symmetric in them: see the file comment), z = x + y and
// pz = phi(z) for the caller; the score is the sum of the return value over the wave (head_sum4)
template <int Q>
__device__ __forceinline__ float gatv2_head_score(const HeadRow<Q>& a, const HeadRow<Q>& x, const HeadRow<Q>& y, float eps,
                                                  HeadRow<Q>& z, HeadRow<Q>& pz) {
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    z.p[q] = x.p[q] + y.p[q];
    const f4 ze = z.p[q] * eps;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pz.p[q][k] = z.p[q][k] > 0.0f ? z.p[q][k] : ze[k];
      t = (q == 0 && k == 0) ? a.p[0][0] * pz.p[0][0] : __builtin_fmaf(a.p[q][k], pz.p[q][k], t);
    }
  }
  return t;
}

// ---- forward: scores, ONLINE softmax and aggregation of a 64-edge chunk ---------------------------------------------------------
// Per batch of U edges: U lane sums, four to a head_sum4 (the DPP wait states once per four edges), the batch maximum FIRST, one
// rescale of (m, l, acc) and U + 1 exponentials, as gatv2_fwd_chunk_kernel.  Every per-edge quantity is wave-uniform: nothing meets
// at the end of a chunk.  Partials in the format of gat_head_fwd_chunk_kernel -- out_partial [n_chunks][len], ms_partial
// [n_chunks] = (m, l) -- for gat_head_fwd_reduce_kernel, which writes out and row_stats.
// DROP: out_i = act(sum_j p_ij w_ij h_j), w = mask . scale of element e of the [ne] array gaib_dropout fills (head_drop_mask: one
// hash per lane and chunk, then a ballot); the weight of a step is a wave-uniform scalar, and m, l and the row statistics do not
// see it.  The three trailing arguments are the DROP form's.
// E: the element type of feat.  A bf16 row is Q loads of 8 bytes (head_load_raw: a load instruction of the wave covers 512
// contiguous bytes), waits packed and is widened exactly (head_widen) behind the batch's sched_barrier; the chunk's own row once.
template <int CPL, int U, bool DROP = false, typename E = float>
__global__ __launch_bounds__(256) void gatv2_head_fwd_chunk_kernel(int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase,
                                                                   const uint32_t* chunk_start, const int64_t* rowptr, const uint32_t* col,
                                                                   const E* feat, const float* a, float eps, float* out_partial,
                                                                   float2* ms_partial, int per_xcd, float drop_rate = 0.0f,
                                                                   float drop_scale = 1.0f, uint64_t drop_seed = 0) {
  static_assert((CPL == 4 || CPL == 8) && U % 4 == 0 && 64 % U == 0, "one head of 256 or 512 columns, four scores per wave sum");
  constexpr int Q = CPL / 4, LEN = 64 * CPL;
  HeadChunk ck;
  if (!head_chunk(n_chunks, chunk_row, chunk_ebase, chunk_start, rowptr, per_xcd, &ck)) return;
  const int lane = threadIdx.x & 63, n = ck.n;
  const int loff = 4 * lane;
  const int cl = (int)col[ck.eb + (lane < n ? lane : 0)];  // (lanes past the end: the chunk's first edge)
  const HeadRow<Q> a4 = head_load<Q>(a + loff);
  const HeadRow<Q> hi = head_widen<Q, E>(head_load_raw<Q, E>(feat + ck.row * (int64_t)LEN + loff));
  uint64_t mb = 0;  // DROP: the masks of the chunk's edges, bit t = step t
  if constexpr (DROP) mb = head_drop_mask(lane, n, (uint64_t)(ck.eb + lane), drop_seed, drop_rate);
  float m = GAT_NEG, l = 0.f;
  HeadRow<Q> acc;
#pragma unroll
  for (int q = 0; q < Q; ++q) acc.p[q] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 64; j += U) {
    if (j >= n) continue;  // (wave-uniform: no edge of the chunk is left)
    HeadRaw<Q, E> xh_raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane(cl, j + u);
      xh_raw[u] = head_load_raw<Q, E>(feat + (int64_t)cj * LEN + loff);
    }
    __builtin_amdgcn_sched_barrier(0);  // all loads of the batch are issued before the first one is consumed
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      HeadRow<Q> z, pz;
      s[u] = gatv2_head_score<Q>(a4, hi, head_widen<Q, E>(xh_raw[u]), eps, z, pz);
    }
#pragma unroll
    for (int u = 0; u < U; u += 4) head_sum4(s[u], s[u + 1], s[u + 2], s[u + 3]);
    float mx = m;
#pragma unroll
    for (int u = 0; u < U; ++u)  // (a step past the end looked at the chunk's first edge: its score takes no part)
      if (j + u < n) mx = s[u] > mx ? s[u] : mx;
    const float sc = __expf(m - mx);  // (the first batch: NEG - mx underflows to 0 on empty sums)
    l *= sc;
#pragma unroll
    for (int q = 0; q < Q; ++q) acc.p[q] *= sc;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j + u < n) {  // (wave-uniform)
        const float e = __expf(s[u] - mx);
        l += e;  // (undropped under DROP too)
        float ew = e;
        if constexpr (DROP) ew = e * (((mb >> (j + u)) & 1u) ? drop_scale : 0.0f);  // (a scalar bit test and select)
        const HeadRow<Q> xh = head_widen<Q, E>(xh_raw[u]);  // (bf16: a second widening, not a copy kept across the batch's maximum)
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
          for (int k = 0; k < 4; ++k) acc.p[q][k] = __builtin_fmaf(ew, xh.p[q][k], acc.p[q][k]);
      }
    }
    m = mx;
  }
  float* po = out_partial + ck.slot * LEN + loff;
#pragma unroll
  for (int q = 0; q < Q; ++q) *reinterpret_cast<f4*>(po + q * 256) = acc.p[q];
  if (lane == 0) ms_partial[ck.slot] = float2{m, l};
}

// ---- backward: the whole input gradient and a's gradient in ONE sweep over the chunks of row j -------------------------------------
// The expressions of gatv2_bwd_chunk_kernel with p_ij, p_ji, ds_ij, ds_ji as wave-uniform scalars: per edge three wave sums -- the
// score, <g_j, h_i> and <g_i, h_j> -- in one head_sum4, then per lane and column
//   acc += p_ij g_i + (ds_ij + ds_ji) a phi'(z)          ag += ds_ji phi(z)
// (a phi'(z) as a times a select between ds and ds eps: no second copy of a in registers).  grad_out leaves as one partial row per
// chunk (gatv2_head_rows_kernel adds them per row in chunk order); ag meets over the workgroup's four waves in LDS, in wave order
// (4 x len floats: 8 KB at 512 columns), and leaves as ONE partial vector per workgroup, agrad_partial [gridDim.x][len].
// Registers at 512 columns: a, h_j, g_j, acc and ag are 40 loop-invariant VGPRs, every edge in flight 16 more (xh, xg).
// DROP: the expressions of gatv2_bwd_chunk_kernel<.., DROP> under two ballots, the chunk's edges' masks (w_ji) and their reverse
// edges' (w_ij, over rev[eb + lane]: one coalesced 256 B per chunk).  The three sums still meet in one head_sum4 and the two dots
// are scaled AFTER it (scale 1: the undropped bits).  Where w_ij = 0 nothing of g_i is used: that step's grad gather is redirected
// to the chunk's own row (a scalar select of the row id ahead of the load, a resident line; the loads of a batch stay
// unconditional), dp_ij is SELECTED to 0 and the p w g term is skipped -- no product with what the redirected load returned
// reaches a result.  The four trailing arguments are the DROP form's.
// E: the element type of feat and grad, as in the forward (bf16 at 512 columns: every edge in flight 8 VGPRs instead of 16).
template <int CPL, int U, bool DROP = false, typename E = float>
__global__ __launch_bounds__(256) void gatv2_head_bwd_chunk_kernel(int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase,
                                                                   const uint32_t* chunk_start, const int64_t* rowptr, const uint32_t* col,
                                                                   const E* feat, const E* grad, const f4* rec, const float* a,
                                                                   float eps, float* out_partial, float* agrad_partial, int per_xcd,
                                                                   const uint32_t* rev = nullptr, float drop_rate = 0.0f,
                                                                   float drop_scale = 1.0f, uint64_t drop_seed = 0) {
  static_assert((CPL == 4 || CPL == 8) && 64 % U == 0, "one head of 256 or 512 columns");
  constexpr int Q = CPL / 4, LEN = 64 * CPL;
  __shared__ float sm[4 * LEN];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int loff = 4 * lane;
  HeadRow<Q> ag;
#pragma unroll
  for (int q = 0; q < Q; ++q) ag.p[q] = f4{0.f, 0.f, 0.f, 0.f};
  HeadChunk ck;
  if (head_chunk(n_chunks, chunk_row, chunk_ebase, chunk_start, rowptr, per_xcd, &ck)) {  // (no early return: the workgroup meets below)
    const int n = ck.n;
    const int cl = (int)col[ck.eb + (lane < n ? lane : 0)];  // (lanes past the end: the chunk's first edge)
    const HeadRow<Q> a4 = head_load<Q>(a + loff);
    const HeadRow<Q> hi = head_widen<Q, E>(head_load_raw<Q, E>(feat + ck.row * (int64_t)LEN + loff));
    const HeadRow<Q> gi = head_widen<Q, E>(head_load_raw<Q, E>(grad + ck.row * (int64_t)LEN + loff));
    const f4 ri = rec[ck.row];  // (delta_j, m_j, 1 / l_j)
    uint64_t mb_e = 0, mb_r = 0;  // DROP: the masks of the chunk's edges and of their reverse edges, bit t = step t
    if constexpr (DROP) {
      mb_e = head_drop_mask(lane, n, (uint64_t)(ck.eb + lane), drop_seed, drop_rate);
      mb_r = head_drop_mask(lane, n, (uint64_t)rev[ck.eb + (lane < n ? lane : 0)], drop_seed, drop_rate);
    }
    HeadRow<Q> acc;
#pragma unroll
    for (int q = 0; q < Q; ++q) acc.p[q] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 64; j += U) {
      if (j >= n) continue;  // (wave-uniform: no edge of the chunk is left)
      HeadRaw<Q, E> xh_raw[U], xg_raw[U];
      f4 rc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane(cl, j + u);
        uint32_t cg = cj;  // DROP: a dropped reverse edge gathers the chunk's own grad row (see above)
        if constexpr (DROP) cg = ((mb_r >> (j + u)) & 1u) ? cj : (uint32_t)ck.row;
        xh_raw[u] = head_load_raw<Q, E>(feat + (int64_t)cj * LEN + loff);
        xg_raw[u] = head_load_raw<Q, E>(grad + (int64_t)cg * LEN + loff);
        rc[u] = rec[cj];
      }
      __builtin_amdgcn_sched_barrier(0);  // all loads of the batch are issued before the first one is consumed
#pragma unroll
      for (int u = 0; u < U; ++u) {
        HeadRow<Q> z, pz;
        const HeadRow<Q> xh = head_widen<Q, E>(xh_raw[u]), xg = head_widen<Q, E>(xg_raw[u]);
        float s = gatv2_head_score<Q>(a4, hi, xh, eps, z, pz);  // the forward's bits, from either end
        float dp_ji = head_dot<Q>(gi, xh), dp_ij = head_dot<Q>(xg, hi), none = 0.f;
        head_sum4(s, dp_ji, dp_ij, none);
        bool keep_ij = true;
        if constexpr (DROP) {
          keep_ij = ((mb_r >> (j + u)) & 1u) != 0;
          dp_ji *= ((mb_e >> (j + u)) & 1u) ? drop_scale : 0.0f;
          dp_ij = keep_ij ? dp_ij * drop_scale : 0.0f;
        }
        const float p_ji = __expf(s - ri[1]) * ri[2];
        const float p_ij = __expf(s - rc[u][1]) * rc[u][2];
        const float ds_ji = p_ji * (dp_ji - ri[0]);
        const float ds_ij = p_ij * (dp_ij - rc[u][0]);
        const float ds = ds_ij + ds_ji, dse = ds * eps;
        float pw_ij = p_ij;  // the gradient flows back along the DROPPED attention p_ij w_ij: nothing where the bit is 0
        if constexpr (DROP) pw_ij = p_ij * drop_scale;
        if (j + u < n) {  // (wave-uniform; a step past the end looked at the chunk's first edge: nothing of it is added)
#pragma unroll
          for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              if (keep_ij) acc.p[q][k] = __builtin_fmaf(pw_ij, xg.p[q][k], acc.p[q][k]);  // (wave-uniform)
              acc.p[q][k] = __builtin_fmaf(z.p[q][k] > 0.0f ? ds : dse, a4.p[q][k], acc.p[q][k]);
              ag.p[q][k] = __builtin_fmaf(ds_ji, pz.p[q][k], ag.p[q][k]);
            }
        }
      }
    }
    float* po = out_partial + ck.slot * LEN + loff;
#pragma unroll
    for (int q = 0; q < Q; ++q) *reinterpret_cast<f4*>(po + q * 256) = acc.p[q];
  }
  // the workgroup's four chunks meet in wave order (a wave without a chunk brings zeros)
#pragma unroll
  for (int q = 0; q < Q; ++q) *reinterpret_cast<f4*>(sm + wv * LEN + q * 256 + loff) = ag.p[q];
  __syncthreads();
  // DROP: the vector is stored at the index of the workgroup's CHUNKS (head_chunk's blk), so a's sum does not depend on the per_xcd
  // walk (gatv2_seq.h)
  int64_t slot_ag = blockIdx.x;
  if constexpr (DROP)
    if (per_xcd > 0) slot_ag = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
#pragma unroll
  for (int t = threadIdx.x; t < LEN; t += 256)
    agrad_partial[slot_ag * LEN + t] = ((sm[t] + sm[LEN + t]) + sm[2 * LEN + t]) + sm[3 * LEN + t];
}

// out[row] = sum of the row's chunk partials in chunk order (gat_head_bwd_reduce_kernel without its pair of sums).  One wave per row.
template <int CPL>
__global__ __launch_bounds__(256) void gatv2_head_rows_kernel(int64_t nv, const uint32_t* chunk_start, const float* out_partial,
                                                              float* out) {
  constexpr int Q = CPL / 4, LEN = 64 * CPL;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const int64_t c0 = chunk_start[row], c1 = chunk_start[row + 1];
  HeadRow<Q> s;
#pragma unroll
  for (int q = 0; q < Q; ++q) s.p[q] = f4{0.f, 0.f, 0.f, 0.f};
  for (int64_t k = c0; k < c1; ++k) {
    const HeadRow<Q> t = head_load<Q>(out_partial + k * LEN + 4 * lane);
#pragma unroll
    for (int q = 0; q < Q; ++q) s.p[q] += t.p[q];
  }
  float* po = out + row * (int64_t)LEN + 4 * lane;
#pragma unroll
  for (int q = 0; q < Q; ++q) *reinterpret_cast<f4*>(po + q * 256) = s.p[q];
}

}  // namespace
