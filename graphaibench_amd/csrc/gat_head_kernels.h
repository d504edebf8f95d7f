// gat_head_kernels.h -- the one-sweep GAT for ONE head of 256 or 512 columns (option gat_fused_head; gat_head.hip instantiates
// these kernels, gat_fused_seq.h holds the host sequence).  A head wider than 128 columns does not fit the group layout of
// gat_kernels.h (a head inside at most 32 lanes, 64 / G edges per step), and column slabs cannot cut it: the score
// a_l.h_i + a_r.h_c and the backward dot <grad_i, h_c> need the whole head.  So here the WHOLE WAVE works on one edge per step:
//   * work split as in the narrow sweeps: one wave per 64-edge chunk of the ordered chunk list, four chunks per workgroup, the
//     per_xcd walk of gat_bwd_fused_chunk_kernel;
//   * a lane owns CPL = len / 64 columns (4 or 8) as Q = CPL / 4 pieces of 16 bytes at columns q 256 + 4 lane, so every load
//     instruction of the wave covers one contiguous 1 KB of a row;
//   * the chunk's 64 column ids are fetched once, one per lane; the id of step t is readlane(ids, t) with t a compile-time
//     constant after unrolling -- a scalar, so a row's base address is scalar arithmetic and the lanes add one loop-invariant
//     offset (the addressing of spmm_core.h's gathers; the row product is taken in 64 bits, tables past 4 GB included).  The column
//     vertex's record (rowdot, M, 1 / S) is wave-uniform too: one 16-byte load per edge;
//   * a dot over the head is a sum over the wave (head_sum): the 16-lane DPP sum of lanes_sum<16>, then two DPP row broadcasts
//     (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3) that leave the total in lane 63, and one v_readlane --
//     seven instructions and a scalar result, where __shfl_xor 16, 32 costs two ds_bpermute, their address and an LDS wait, and
//     v_permlane32_swap needs a copy per swap.  Every quantity per edge (scores, attention, the softmax state) is therefore
//     wave-uniform, and with one edge per step there is no group merge at the end of a chunk;
//   * U edges in flight: all loads of a batch are issued before the first is consumed (sched_barrier).  The end of a chunk is
//     wave-uniform, so a whole batch past the end is skipped; inside the last batch the steps past the end read the chunk's FIRST
//     edge (the lanes past the end hold its id) and are skipped at the point of use: a dummy read reaches no output.
// Forward: the online softmax of gat_fwd_fused_chunk_kernel (GAT_NEG, one __expf per edge, the same rescaling), partials
// out_partial [n_chunks][len] and ms_partial [n_chunks]; gat_head_fwd_reduce_kernel is gat_fwd_reduce_kernel's mathematics.  Its
// scores and its running maximum are fp64 (head_dot64, head_sum64 below: the reason stands there).
// Backward: the RECOMP form of gat_bwd_fused_chunk_kernel (its expressions for dse, dsr, ge, gr), partial output row and partial
// (s_e, s_r) per chunk, added per row in chunk order by gat_head_bwd_reduce_kernel.  rowdot_kernel, gat_rec_kernel and the alpha
// reduction are the narrow calls' own (none of them has a width limit below 512: alpha_partial_kernel walks a row in passes of 256
// columns over its 512 floats of LDS).  Deterministic, no atomics; every store is a plain vector store.
// ld / rec_ld / stats_ld: row strides of the tables (floats), of the records (16-byte records) and of the statistics (float2
// records), taken as arguments so that a later change can run heads of these widths as slabs of a wider row.
#pragma once
#include "gat_kernels.h"

namespace {

// this lane's Q pieces of 16 bytes of a row: columns q 256 + 4 lane
template <int Q>
struct HeadRow {
  f4 p[Q];
};
template <int Q>
__device__ __forceinline__ HeadRow<Q> head_load(const float* row_lane_ptr) {
  HeadRow<Q> r;
#pragma unroll
  for (int q = 0; q < Q; ++q) r.p[q] = *reinterpret_cast<const f4*>(row_lane_ptr + q * 256);
  return r;
}
// the same pieces AS LOADED from a table of element type E (Row4<E>::Raw: 16 bytes of fp32, 8 bytes of raw bf16 bits -- columns
// q 256 + 4 lane are then one 8-byte load and a load instruction of the wave covers one contiguous 512 B): a gathered row waits
// packed, half the registers per row in flight, and is widened exactly (Row4<E>::widen) where it is consumed, behind the batch's
// sched_barrier.  For E = float both are the identity and the kernels are the fp32 kernels as they were.
template <int Q, typename E>
struct HeadRaw {
  typename Row4<E>::Raw p[Q];
};
template <int Q, typename E>
__device__ __forceinline__ HeadRaw<Q, E> head_load_raw(const E* row_lane_ptr) {
  HeadRaw<Q, E> r;
#pragma unroll
  for (int q = 0; q < Q; ++q) r.p[q] = load_row4(row_lane_ptr + q * 256);
  return r;
}
template <int Q, typename E>
__device__ __forceinline__ HeadRow<Q> head_widen(const HeadRaw<Q, E>& r) {
  HeadRow<Q> w;
#pragma unroll
  for (int q = 0; q < Q; ++q) w.p[q] = Row4<E>::widen(r.p[q]);
  return w;
}
// <a, b> over this lane's columns: one FMA chain through the pieces (d4's order inside a piece)
template <int Q>
__device__ __forceinline__ float head_dot(const HeadRow<Q>& a, const HeadRow<Q>& b) {
  float s = a.p[0][0] * b.p[0][0];
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int k = (q == 0 ? 1 : 0); k < 4; ++k) s = __builtin_fmaf(a.p[q][k], b.p[q][k], s);
  return s;
}
// a, b, c, d <- their sums over the wave in a fixed order, as wave-uniform values (see the file comment).  Four at a time, inline:
// the compiler folds no row broadcast under a row mask into the add (it emits a zeroing move, v_mov_b32_dpp and the add), and the
// two wait states a DPP operand needs behind the VALU write of its register are paid once per stage, not once per value -- a
// later stage reads registers written four instructions earlier (the scheme of lanes_sum4_dpp).  A row that a row mask leaves out
// keeps its value.  Not volatile: the block has no effect beyond its four registers, and a volatile one would count as a store
// and take the records' loads off the scalar path.
__device__ __forceinline__ void head_sum4(float& a, float& b, float& c, float& d) {
#define GAIB_HS4(CTRL)                                  \
  "v_add_f32_dpp %0, %0, %0 " CTRL " bank_mask:0xf\n\t" \
  "v_add_f32_dpp %1, %1, %1 " CTRL " bank_mask:0xf\n\t" \
  "v_add_f32_dpp %2, %2, %2 " CTRL " bank_mask:0xf\n\t" \
  "v_add_f32_dpp %3, %3, %3 " CTRL " bank_mask:0xf\n\t"
  asm("s_nop 1\n\t"                                  //
      GAIB_HS4("quad_perm:[1,0,3,2] row_mask:0xf")   // the 16-lane rows, as lanes_sum<16>
      GAIB_HS4("quad_perm:[2,3,0,1] row_mask:0xf")   //
      GAIB_HS4("row_half_mirror row_mask:0xf")       //
      GAIB_HS4("row_mirror row_mask:0xf")            //
      GAIB_HS4("row_bcast:15 row_mask:0xa")          // rows 1 and 3 add the total of the row before them
      GAIB_HS4("row_bcast:31 row_mask:0xc")          // rows 2 and 3 add the total of rows 0 and 1: lane 63 has all four rows
      "s_nop 0"
      : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#undef GAIB_HS4
  a = readlane_f(a, 63), b = readlane_f(b, 63), c = readlane_f(c, 63), d = readlane_f(d, 63);
}
// the row's own dots: two values, rarely
__device__ __forceinline__ void head_sum2(float& a, float& b) {
  float z0 = 0.f, z1 = 0.f;
  head_sum4(a, b, z0, z1);
}

// The forward's scores in fp64.  A score reaches +-100 here, where fp32 resolves 7.6e-6, and a row of the `underflow` kind hands
// that error to its attention whole: the output's small entries then lie 3.7e-4 (256 columns) and 9.2e-4 (512) from fp64, past
// twice the fp32 oracle's own distance.  Neither the sum a_l.h_i + a_r.h_c alone (256) nor the dots alone (512) account for it, so
// both are taken in fp64 -- v_fma_f64 and v_add_f64 run at the fp32 rate on this part -- and the online softmax keeps its maximum in
// fp64; only the argument of the exponential, a difference, is rounded to fp32.
// <a, b> over this lane's columns: the products of two fp32 are exact in fp64
template <int Q>
__device__ __forceinline__ double head_dot64(const HeadRow<Q>& a, const HeadRow<Q>& b) {
  double s = (double)a.p[0][0] * (double)b.p[0][0];
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int k = (q == 0 ? 1 : 0); k < 4; ++k) s = __builtin_fma((double)a.p[q][k], (double)b.p[q][k], s);
  return s;
}
// v of another lane by a DPP control; the rows that ROW_MASK leaves out read 0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double head_dpp64(double v) {
  const uint64_t b = (uint64_t)__builtin_bit_cast(int64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, ROW_MASK, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, ROW_MASK, 0xf, false);
  return __builtin_bit_cast(double, (int64_t)(((uint64_t)hi << 32) | lo));
}
// the sum of v over the wave, wave-uniform: head_sum4's six stages (the same controls, the same order) on one fp64 value
__device__ __forceinline__ double head_sum64(double v) {
  v += head_dpp64<0xB1, 0xf>(v);   // quad_perm:[1,0,3,2]
  v += head_dpp64<0x4E, 0xf>(v);   // quad_perm:[2,3,0,1]
  v += head_dpp64<0x141, 0xf>(v);  // row_half_mirror
  v += head_dpp64<0x140, 0xf>(v);  // row_mirror
  v += head_dpp64<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v += head_dpp64<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3: lane 63 has all four rows
  const uint64_t b = (uint64_t)__builtin_bit_cast(int64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), 63);
  return __builtin_bit_cast(double, (int64_t)(((uint64_t)hi << 32) | lo));
}

// the chunk of this wave: its row, first edge, edge count and slot among the row's chunks -- the same in every lane, and said so
// (readfirstlane): the end of the chunk is then a scalar comparison and the row's own addresses scalar arithmetic
__device__ __forceinline__ int64_t head_uniform(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
struct HeadChunk {
  int64_t row, eb, slot;
  int n;
};
__device__ __forceinline__ bool head_chunk(int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase,
                                           const uint32_t* chunk_start, const int64_t* rowptr, int per_xcd, HeadChunk* ck) {
  int64_t blk = blockIdx.x;  // (per_xcd: see gat_bwd_fused_chunk_kernel)
  if (per_xcd > 0) blk = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  const int64_t c = blk * 4 + (threadIdx.x >> 6);
  if (c >= n_chunks) return false;
  const int64_t row = chunk_row[c], eb = chunk_ebase[c];
  const int64_t rem = rowptr[row + 1] - eb;
  ck->row = head_uniform(row);
  ck->eb = head_uniform(eb);
  ck->n = __builtin_amdgcn_readfirstlane(rem < 64 ? (int)rem : 64);
  ck->slot = head_uniform((int64_t)chunk_start[row] + (eb - rowptr[row]) / 64);
  return true;
}

// DROP: the masks of the chunk's 64 edges as one wave-uniform 64-bit word, bit t = step t.  With one head the mask of edge e is
// element e of the [ne] array gaib_dropout fills under the same seed, u01(seed, e) > rate, and the wave is on one edge per step:
// lane t hashes the index it is handed ONCE, ahead of the edge loop (the chunk's own edge eb + t; in backward also rev[eb + t]), and
// a ballot leaves the 64 bits in a scalar pair -- lanes past the end of the chunk contribute 0.  In the loop the weight of step t
// is a scalar bit test against a compile-time t and a select between scale and 0: one hash per lane and chunk, where
// gat_drop_bits shares a head's steps among its lanes and ORs them together.
__device__ __forceinline__ uint64_t head_drop_mask(int lane, int n, uint64_t index, uint64_t seed, float rate) {
  return __ballot(lane < n && u01_of_key(u01_key(seed, index)) > rate);  // (the index in 64 bits, as gaib_dropout's)
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// E: the element type of feat.  DROP: out_i = sum_e p_e w_e h_c with w = mask . scale (head_drop_mask); the running sum, the maximum
// and so the row statistics do not see the mask.  The three trailing arguments are the DROP form's.
template <int CPL, int U, typename E = float, bool DROP = false>
__global__ __launch_bounds__(256) void gat_head_fwd_chunk_kernel(int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase,
                                                                 const uint32_t* chunk_start, const int64_t* rowptr, const uint32_t* col,
                                                                 const E* feat, int ld, const float* alpha_l, const float* alpha_r,
                                                                 float eps, float* out_partial, float2* ms_partial, int per_xcd,
                                                                 float drop_rate = 0.0f, float drop_scale = 1.0f, uint64_t drop_seed = 0) {
  static_assert((CPL == 4 || CPL == 8) && 64 % U == 0, "one head of 256 or 512 columns");
  constexpr int Q = CPL / 4, LEN = 64 * CPL;
  HeadChunk ck;
  if (!head_chunk(n_chunks, chunk_row, chunk_ebase, chunk_start, rowptr, per_xcd, &ck)) return;
  const int lane = threadIdx.x & 63, n = ck.n;
  const int loff = 4 * lane;
  const int cl = (int)col[ck.eb + (lane < n ? lane : 0)];  // (lanes past the end: the chunk's first edge)
  const HeadRow<Q> ar = head_load<Q>(alpha_r + loff);
  const double sl_i =
      head_sum64(head_dot64<Q>(head_load<Q>(alpha_l + loff), head_widen<Q, E>(head_load_raw<Q, E>(feat + ck.row * (int64_t)ld + loff))));
  uint64_t mb = 0;
  if constexpr (DROP) mb = head_drop_mask(lane, n, (uint64_t)(ck.eb + lane), drop_seed, drop_rate);
  const double eps64 = (double)eps;
  double m = (double)GAT_NEG;  // (fp64: see head_dot64)
  float ssum = 0.f;
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
      xh_raw[u] = head_load_raw<Q, E>(feat + (int64_t)cj * ld + loff);
    }
    __builtin_amdgcn_sched_barrier(0);  // all loads of the batch are issued before the first one is consumed
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const HeadRow<Q> xh = head_widen<Q, E>(xh_raw[u]);
      const double sr_c = head_sum64(head_dot64<Q>(ar, xh));
      if (j + u < n) {  // (wave-uniform; a step past the end looked at the chunk's first edge: nothing of it is added)
        const double t0 = sl_i + sr_c;
        const double t = t0 > 0.0 ? t0 : eps64 * t0;
        // online softmax: one of exp(m - max), exp(t - max) is exp(0) -- ONE exponential per edge
        const float d = (float)(t - m);
        const float ex = __expf(d > 0.f ? -d : d);
        const float sc = d > 0.f ? ex : 1.f, e = d > 0.f ? 1.f : ex;
        ssum = __builtin_fmaf(ssum, sc, e);
        float ew = e;
        if constexpr (DROP) ew = e * (((mb >> (j + u)) & 1u) ? drop_scale : 0.0f);  // (a scalar bit test and select)
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
          for (int k = 0; k < 4; ++k) acc.p[q][k] = __builtin_fmaf(ew, xh.p[q][k], acc.p[q][k] * sc);
        m = d > 0.f ? t : m;
      }
    }
  }
  // the partial goes out relative to the fp32 maximum it is stored with: exp(m - mf) = 1 + (m - mf) to 2^-48
  const float mf = (float)m;
  const float fix = 1.0f + (float)(m - (double)mf);
  ssum *= fix;
  float* po = out_partial + ck.slot * LEN + loff;
#pragma unroll
  for (int q = 0; q < Q; ++q) *reinterpret_cast<f4*>(po + q * 256) = acc.p[q] * fix;
  if (lane == 0) ms_partial[ck.slot] = float2{mf, ssum};
}

// per row: combine the chunks' (m, s, acc) in chunk order; out = act(sum / S); stats[row] = (M, 1 / S).  One wave per row.
template <int CPL>
__global__ __launch_bounds__(256) void gat_head_fwd_reduce_kernel(int64_t nv, const uint32_t* chunk_start, const float* out_partial,
                                                                  const float2* ms_partial, int relu, float* out, int ld, float2* stats,
                                                                  int stats_ld) {
  constexpr int Q = CPL / 4, LEN = 64 * CPL;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const int64_t c0 = chunk_start[row], c1 = chunk_start[row + 1];
  float M = GAT_NEG;
  for (int64_t k = c0 + lane; k < c1; k += 64) {
    const float mk = ms_partial[k].x;
    M = mk > M ? mk : M;
  }
  M = wave_max(M);
  float S = 0.f;
  HeadRow<Q> s;
#pragma unroll
  for (int q = 0; q < Q; ++q) s.p[q] = f4{0.f, 0.f, 0.f, 0.f};
  for (int64_t k = c0; k < c1; ++k) {
    const float2 ms = ms_partial[k];
    const float w = __expf(ms.x - M);
    S += ms.y * w;
    const HeadRow<Q> t = head_load<Q>(out_partial + k * LEN + 4 * lane);
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) s.p[q][i] += t.p[q][i] * w;
  }
  const float inv = S > 0.f ? 1.0f / S : 0.f;
  float* po = out + row * (int64_t)ld + 4 * lane;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s.p[q][i] *= inv;
      if (relu) s.p[q][i] = s.p[q][i] > 0.f ? s.p[q][i] : 0.f;
    }
    *reinterpret_cast<f4*>(po + q * 256) = s.p[q];
  }
  if (lane == 0) stats[row * stats_ld] = float2{M, inv};
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// rec: (rowdot, row maximum, 1 / row sum, 0) per vertex (gat_rec_kernel), rows of rec_ld records
// E: the element type of feat and grad.  DROP: the expressions of gat_bwd_fused_chunk_kernel<.., DROP = true> -- dp_e = w_e <grad_i,
// h_c>, dp_r = w_r <grad_c, h_i>, out_i += p_r w_r grad_c with r = rev(e) -- under two masks, the chunk's edges' and their reverse
// edges' (rev: one coalesced 256 B per chunk).  Where the reverse edge is dropped nothing of grad_c is used, so that step's grad
// gather is REDIRECTED to the chunk's own row (a scalar select of the row id ahead of the load: a line that is resident instead
// of one from HBM; the loads of a batch stay unconditional, the vmcnt waits exact) and dp_r and the weight of grad_c are SELECTED
// to 0 on the bit -- no product with what the redirected load returned reaches a result.  The four trailing arguments are the
// DROP form's.
template <int CPL, int U, typename E = float, bool DROP = false>
__global__ __launch_bounds__(256) void gat_head_bwd_chunk_kernel(int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase,
                                                                 const uint32_t* chunk_start, const int64_t* rowptr, const uint32_t* col,
                                                                 const E* feat, const E* grad, int ld, const f4* rec, int rec_ld,
                                                                 const float* alpha_l, const float* alpha_r, float eps,
                                                                 float* out_partial, float* rc_partial, int per_xcd,
                                                                 const uint32_t* rev = nullptr, float drop_rate = 0.0f,
                                                                 float drop_scale = 1.0f, uint64_t drop_seed = 0) {
  static_assert((CPL == 4 || CPL == 8) && 64 % U == 0, "one head of 256 or 512 columns");
  constexpr int Q = CPL / 4, LEN = 64 * CPL;
  HeadChunk ck;
  if (!head_chunk(n_chunks, chunk_row, chunk_ebase, chunk_start, rowptr, per_xcd, &ck)) return;
  const int lane = threadIdx.x & 63, n = ck.n;
  const int loff = 4 * lane;
  const int cl = (int)col[ck.eb + (lane < n ? lane : 0)];  // (lanes past the end: the chunk's first edge)
  const HeadRow<Q> gi = head_widen<Q, E>(head_load_raw<Q, E>(grad + ck.row * (int64_t)ld + loff));
  const HeadRow<Q> hi = head_widen<Q, E>(head_load_raw<Q, E>(feat + ck.row * (int64_t)ld + loff));
  uint64_t mb_e = 0, mb_r = 0;  // DROP: the masks of the chunk's edges and of their reverse edges
  if constexpr (DROP) {
    mb_e = head_drop_mask(lane, n, (uint64_t)(ck.eb + lane), drop_seed, drop_rate);
    mb_r = head_drop_mask(lane, n, (uint64_t)rev[ck.eb + (lane < n ? lane : 0)], drop_seed, drop_rate);
  }
  const HeadRow<Q> al = head_load<Q>(alpha_l + loff), ar = head_load<Q>(alpha_r + loff);
  // the per-vertex dots a_l.h_v, a_r.h_v are formed again from the gathered rows; only rowdot comes from a table
  float sl_i = head_dot<Q>(al, hi), sr_i = head_dot<Q>(ar, hi);
  head_sum2(sl_i, sr_i);
  const f4 ri = rec[ck.row * rec_ld];
  const float rd_i = ri[0], m_i = ri[1], is_i = ri[2];
  HeadRow<Q> acc;
#pragma unroll
  for (int q = 0; q < Q; ++q) acc.p[q] = f4{0.f, 0.f, 0.f, 0.f};
  float s_e = 0.f, s_r = 0.f;
#pragma unroll
  for (int j = 0; j < 64; j += U) {
    if (j >= n) continue;  // (wave-uniform: no edge of the chunk is left)
    HeadRaw<Q, E> xg_raw[U], xh_raw[U];
    f4 rc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane(cl, j + u);
      uint32_t cg = cj;  // DROP: a dropped reverse edge gathers the chunk's own grad row (see above)
      if constexpr (DROP) cg = ((mb_r >> (j + u)) & 1u) ? cj : (uint32_t)ck.row;
      xg_raw[u] = head_load_raw<Q, E>(grad + (int64_t)cg * ld + loff);
      xh_raw[u] = head_load_raw<Q, E>(feat + (int64_t)cj * ld + loff);
      rc[u] = rec[(int64_t)cj * rec_ld];
    }
    __builtin_amdgcn_sched_barrier(0);  // all loads of the batch are issued before the first one is consumed
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const HeadRow<Q> xg = head_widen<Q, E>(xg_raw[u]), xh = head_widen<Q, E>(xh_raw[u]);
      float dpe = head_dot<Q>(gi, xh), dpr = head_dot<Q>(xg, hi), sl_c = head_dot<Q>(al, xh), sr_c = head_dot<Q>(ar, xh);
      head_sum4(dpe, dpr, sl_c, sr_c);
      bool keep_r = true;
      if constexpr (DROP) {
        keep_r = ((mb_r >> (j + u)) & 1u) != 0;
        dpe *= ((mb_e >> (j + u)) & 1u) ? drop_scale : 0.0f;
        dpr = keep_r ? dpr * drop_scale : 0.0f;
      }
      const float t_e = sl_i + sr_c, t_r = sl_c + sr_i;  // pre-activation scores of (i -> c) and (c -> i)
      const float a = __expf((t_e > 0.0f ? t_e : eps * t_e) - m_i) * is_i;
      const float b = __expf((t_r > 0.0f ? t_r : eps * t_r) - rc[u][1]) * rc[u][2];
      const float dse = a * (1.0f - a) * dpe - (rd_i - a * dpe) * a;
      const float dsr = b * (1.0f - b) * dpr - (rc[u][0] - b * dpr) * b;
      const float ge = dse * (t_e > 0.0f ? 1.0f : eps);  // leaky-relu' at the score of (i -> c)
      const float gr = dsr * (t_r > 0.0f ? 1.0f : eps);  //              at the score of (c -> i)
      if (j + u < n) {  // (wave-uniform; a step past the end looked at the chunk's first edge: nothing of it is added)
        s_e += ge;
        s_r += gr;
        if constexpr (DROP) {  // the gradient flows back along the DROPPED attention p_r w_r: nothing where the bit is 0
          if (keep_r) {
            const float bw = b * drop_scale;
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
              for (int k = 0; k < 4; ++k) acc.p[q][k] = __builtin_fmaf(bw, xg.p[q][k], acc.p[q][k]);
          }
        } else {
#pragma unroll
          for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc.p[q][k] = __builtin_fmaf(b, xg.p[q][k], acc.p[q][k]);
        }
      }
    }
  }
  float* po = out_partial + ck.slot * LEN + loff;
#pragma unroll
  for (int q = 0; q < Q; ++q) *reinterpret_cast<f4*>(po + q * 256) = acc.p[q];
  if (lane == 0) *reinterpret_cast<float2*>(rc_partial + ck.slot * 2) = float2{s_e, s_r};  // partial row / column sum of g
}

// out[row] = sum of the row's chunk partials in chunk order; rs / cs [row] the same for the g sums.  One wave per row.
template <int CPL>
__global__ __launch_bounds__(256) void gat_head_bwd_reduce_kernel(int64_t nv, const uint32_t* chunk_start, const float* out_partial,
                                                                  const float* rc_partial, float* out, int ld, float* rs, float* cs) {
  constexpr int Q = CPL / 4, LEN = 64 * CPL;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const int64_t c0 = chunk_start[row], c1 = chunk_start[row + 1];
  HeadRow<Q> s;
#pragma unroll
  for (int q = 0; q < Q; ++q) s.p[q] = f4{0.f, 0.f, 0.f, 0.f};
  float r_e = 0.f, r_r = 0.f;
  for (int64_t k = c0; k < c1; ++k) {
    const float2 rc = *reinterpret_cast<const float2*>(rc_partial + k * 2);
    r_e += rc.x;
    r_r += rc.y;
    const HeadRow<Q> t = head_load<Q>(out_partial + k * LEN + 4 * lane);
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) s.p[q][i] += t.p[q][i];
  }
  float* po = out + row * (int64_t)ld + 4 * lane;
#pragma unroll
  for (int q = 0; q < Q; ++q) *reinterpret_cast<f4*>(po + q * 256) = s.p[q];
  if (lane == 0) {
    rs[row] = r_e;
    cs[row] = r_r;
  }
}

}  // namespace
