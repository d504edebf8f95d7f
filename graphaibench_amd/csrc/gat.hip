// gat.hip -- GAT attention kernels for gfx950: edge scores + edge-softmax, SDDMM,
// softmax-backward + alpha gradients, symmetric edge transpose.  All kernels take a head count H
// (the reference is single-head, H = 1; H > 1 = H independent single-head attentions on the column
// slices [h*D/H, (h+1)*D/H), edge arrays laid out [ne][H]).
//
// replaces GAT_Aggregator::aggregate / d_aggregate (src/gnn/gconv/gat_aggregator.cpp:57-200)
// and the CUDA kernels compute_attn_score_warp, compute_scores_grad_warp,
// compute_alpha_grad_warp, symmetric_csr_transpose_kernel
// (include/gnn/graph_operations.h:191-467).
//
// Differences in HOW (results agree to fp32 rounding):
//   * a_l.h[i] and a_r.h[j] are computed once per VERTEX (O(N*D)) and gathered per edge
//     (4 B per head) instead of recomputing a_r.h[col_e] per EDGE (O(E*D), gat_aggregator.cpp:71).
//   * SDDMM is edge-parallel over 64-edge chunks (balanced on power-law rows).
//   * the alpha gradients  sum_e g_e*h[col_e]  and  sum_i (sum_e g_e)*h[i]  are regrouped by
//     vertex using the reverse-edge permutation:  alpha_r' = sum_v cs[v]*h[v],
//     alpha_l' = sum_v rs[v]*h[v]  with rs = row sums and cs = column sums of g
//     (O(E + N*D) instead of O(E*D)); reduction is a fixed two-level tree, no float atomics.
//   * the transposed-score SpMM reads p[rev(e)] directly (gaib_spmm GAIB_W_EDGE_T); the
//     reverse-edge permutation is built once per graph instead of a binary search per call.
#include "common.h"
#include "gat_kernels.h"

namespace {

// s[v,h] = <alpha[slice h], x[v, slice h]> for two alpha vectors at once.  One wave per row.
__global__ __launch_bounds__(256) void vertex_dots_kernel(int64_t nv, int len, int H, const float* x,
                                                          const float* al, const float* ar,
                                                          float* sl, float* sr) {
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * (int64_t)len;
  const int dh = len / H;
  if (H > 1 && dh <= 64 && (64 % dh) == 0) {
    // head slices of 1..64 columns that tile a wave: every 64-column chunk holds whole heads, reduced inside their
    // groups of dh lanes (8 heads x 8 columns: 6 shuffles per row instead of 96)
    for (int c0 = 0; c0 < len; c0 += 64) {
      const int c = c0 + lane;
      const bool ok = c < len;
      const float v = ok ? xr[c] : 0.f;
      float pl = ok ? al[c] * v : 0.f, pr = ok ? ar[c] * v : 0.f;
      for (int o = dh >> 1; o >= 1; o >>= 1) {
        pl += __shfl_xor(pl, o, 64);
        pr += __shfl_xor(pr, o, 64);
      }
      if (ok && (lane % dh) == 0) {
        sl[row * H + c / dh] = pl;
        sr[row * H + c / dh] = pr;
      }
    }
    return;
  }
  for (int h = 0; h < H; ++h) {
    float pl = 0.f, pr = 0.f;
    for (int c = h * dh + lane; c < (h + 1) * dh; c += 64) {
      const float v = xr[c];
      pl += al[c] * v;
      pr += ar[c] * v;
    }
    pl = wave_sum(pl);
    pr = wave_sum(pr);
    if (lane == 0) {
      sl[row * H + h] = pl;
      sr[row * H + h] = pr;
    }
  }
}

// per (row, head): temp = sl[i,h] + sr[col,h]; scores = leaky_relu; norm = softmax over the row.
// (gat_aggregator.cpp:64-77; softmax math_functions.cpp:485-494: max-subtracted, expf, divide)
__global__ __launch_bounds__(256) void edge_softmax_kernel(int64_t nv, int H, const int64_t* rowptr,
                                                           const uint32_t* col, const float* sl,
                                                           const float* sr, float eps, float* temp,
                                                           float* scores, float* norm) {
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
  if (e0 == e1) return;
  if (e1 - e0 <= 64) {
    // whole row in registers, one lane per edge
    const int64_t e = e0 + lane;
    const bool ok = e < e1;
    const int64_t c = ok ? (int64_t)col[e] : 0;
    for (int h = 0; h < H; ++h) {
      float s = -INFINITY;
      if (ok) {
        const float t = sl[row * H + h] + sr[c * H + h];
        temp[e * H + h] = t;
        s = t > 0.0f ? t : eps * t;
        scores[e * H + h] = s;
      }
      const float mx = wave_max(s);
      const float ex = ok ? expf(s - mx) : 0.f;
      const float den = wave_sum(ex);
      if (ok) norm[e * H + h] = ex / den;
    }
    return;
  }
  for (int h = 0; h < H; ++h) {
    const float s_src = sl[row * H + h];
    float mx = -INFINITY;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const float t = s_src + sr[(int64_t)col[e] * H + h];
      temp[e * H + h] = t;
      const float s = t > 0.0f ? t : eps * t;
      scores[e * H + h] = s;
      mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float den = 0.f;
    for (int64_t e = e0 + lane; e < e1; e += 64) {  // each lane re-reads only its own writes
      const float ex = expf(scores[e * H + h] - mx);
      norm[e * H + h] = ex;
      den += ex;
    }
    den = wave_sum(den);
    for (int64_t e = e0 + lane; e < e1; e += 64) norm[e * H + h] = norm[e * H + h] / den;
  }
}

// SDDMM fallback: out[e,h] = <grad[i, slice h], feat[col_e, slice h]>.  One wave per row, one wave
// reduction per (edge, head).  Used for shapes the chunk kernels below do not cover.
__global__ __launch_bounds__(256) void sddmm_generic_kernel(int64_t nv, int H, const int64_t* rowptr,
                                                            const uint32_t* col, int len,
                                                            const float* grad, const float* feat,
                                                            float* out_e) {
  int row32 = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (row32 >= nv) return;
  const int64_t row = __builtin_amdgcn_readfirstlane(row32);  // wave-uniform -> scalar loads
  const int lane = threadIdx.x & 63;
  const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
  const float* gr = grad + row * (int64_t)len;
  const int dh = len / H;
  for (int64_t e = e0; e < e1; ++e) {
    const float* fr = feat + (int64_t)col[e] * len;
    for (int h = 0; h < H; ++h) {
      float p = 0.f;
      for (int c = h * dh + lane; c < (h + 1) * dh; c += 64) p += gr[c] * fr[c];
      p = wave_sum(p);
      if (lane == 0) out_e[e * H + h] = p;
    }
  }
}

// SDDMM, edge-parallel: one wave per 64-edge chunk (gaib_graph_ensure_chunks), G lanes x float4 per
// edge, so one wave instruction gathers 64/G feature rows (1 KB) and a dot product costs
// 4 FMAs + log2 shuffles.  Group k of the wave owns edges k*G .. k*G+G-1 of the chunk; in step
// j it reduces its j-th edge.
//   single head (LH == G): lane k*G+j (which sits in group k) keeps the result, so after G steps
//     lane l holds edge l and the store is coalesced.
//   H heads (LH = lanes per head = (len/H)/4 < G): the reduction stops at LH lanes; the first lane
//     of every head subgroup stores out[e,h] directly.
template <int G, int U, int LH>
__global__ __launch_bounds__(256) void sddmm_chunk_kernel(int64_t n_chunks, const uint32_t* chunk_row,
                                                          const uint32_t* chunk_ebase,
                                                          const int64_t* rowptr, const uint32_t* col,
                                                          int len, int H, const float* grad,
                                                          const float* feat, float* out_e) {
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const int sl = lane & (G - 1), gbase = lane & ~(G - 1);
  const int64_t row = chunk_row[c];
  const int64_t eb = chunk_ebase[c];
  const int64_t rem = rowptr[row + 1] - eb;
  const int n = rem < 64 ? (int)rem : 64;
  const uint32_t cl = col[eb + (lane < n ? lane : 0)];
  const bool colok = sl * 4 < len;
  const int coff = colok ? sl * 4 : 0;
  f4 g4 = {0.f, 0.f, 0.f, 0.f};
  if (colok) g4 = *reinterpret_cast<const f4*>(grad + row * (int64_t)len + coff);
  float res = 0.f;
#pragma unroll
  for (int j = 0; j < G; j += U) {
    f4 x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t cj = (uint32_t)__shfl((int)cl, gbase + j + u, 64);
      x[u] = *reinterpret_cast<const f4*>(feat + (int64_t)cj * len + coff);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float p = g4[0] * x[u][0] + g4[1] * x[u][1] + g4[2] * x[u][2] + g4[3] * x[u][3];
#pragma unroll
      for (int o = LH / 2; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
      if constexpr (LH == G) {
        if (sl == j + u) res = p;
      } else {
        const int ei = gbase + j + u;  // edge index inside the chunk handled by this group now
        if (colok && (sl & (LH - 1)) == 0 && ei < n) out_e[(eb + ei) * H + sl / LH] = p;
      }
    }
  }
  if constexpr (LH == G) {
    if (lane < n) out_e[eb + lane] = res;
  }
}

// softmax backward per (row, head) (math_functions.cpp:496-514, closed form of the :497-504
// branch) + leaky-relu' (gat_aggregator.cpp:145).  Writes ds into scores[], g into gbuf[], and the
// row sum of g into rs[].
__global__ __launch_bounds__(256) void softmax_bwd_kernel(int64_t nv, int H, const int64_t* rowptr,
                                                          const float* p, const float* dp,
                                                          const float* temp, float eps,
                                                          float* scores, float* gbuf, float* rs) {
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
  for (int h = 0; h < H; ++h) {
    float dot = 0.f;
    for (int64_t e = e0 + lane; e < e1; e += 64) dot += p[e * H + h] * dp[e * H + h];
    dot = wave_sum(dot);
    float gs = 0.f;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const float pe = p[e * H + h], dpe = dp[e * H + h];
      const float x = pe * (1.0f - pe) * dpe;
      const float ds = x - (dot - pe * dpe) * pe;
      scores[e * H + h] = ds;
      const float ge = ds * (temp[e * H + h] > 0.0f ? 1.0f : eps);
      gbuf[e * H + h] = ge;
      gs += ge;
    }
    gs = wave_sum(gs);
    if (lane == 0) rs[row * H + h] = gs;
  }
}

// cs[v,h] = sum_{e in row v} g[rev[e],h]  == column sum of g (structurally symmetric graph)
__global__ __launch_bounds__(256) void colsum_kernel(int64_t nv, int H, const int64_t* rowptr,
                                                     const uint32_t* rev, const float* gbuf,
                                                     float* cs) {
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
  for (int h = 0; h < H; ++h) {
    float s = 0.f;
    for (int64_t e = e0 + lane; e < e1; e += 64) s += gbuf[(int64_t)rev[e] * H + h];
    s = wave_sum(s);
    if (lane == 0) cs[row * H + h] = s;
  }
}

__global__ void edge_gather_kernel(int64_t ne, int H, const uint32_t* rev, const float* in, float* out) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ne * H) return;
  const int64_t e = t / H;
  const int h = (int)(t - e * H);
  out[t] = in[(int64_t)rev[e] * H + h];
}

// ---- head-vectorised variants (H in {2,4,8,16}): one lane owns ALL heads of an edge, so the
// [ne][H] arrays are read and written as contiguous 4*H-byte records (the runtime-H kernels above
// walk them with a 4*H-byte stride, 8x the traffic at H = 8) and row reductions run once per row.
template <int H>
struct HeadVec {
  float v[H];
  __device__ __forceinline__ void load(const float* p) {
    if constexpr (H % 4 == 0) {
#pragma unroll
      for (int k = 0; k < H / 4; ++k) {
        const f4 t = reinterpret_cast<const f4*>(p)[k];
        v[4 * k] = t[0]; v[4 * k + 1] = t[1]; v[4 * k + 2] = t[2]; v[4 * k + 3] = t[3];
      }
    } else {
#pragma unroll
      for (int k = 0; k < H; ++k) v[k] = p[k];
    }
  }
  __device__ __forceinline__ void store(float* p) const {
    if constexpr (H % 4 == 0) {
#pragma unroll
      for (int k = 0; k < H / 4; ++k) {
        f4 t = {v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
        reinterpret_cast<f4*>(p)[k] = t;
      }
    } else {
#pragma unroll
      for (int k = 0; k < H; ++k) p[k] = v[k];
    }
  }
};

// Row-owner kernels.  BLK = false: one wave per row, 4 rows per 256-thread block, rows longer than
// heavy_thr are left to the BLK = true launch: one 1024-thread workgroup per heavy row (longest
// first), partial reductions meet in LDS.  A row's edges are strided over the owner's lanes.
constexpr int ROW_BLK_WAVES = 16;

// How a row owner's threads cover the [edge][head] records: a thread handles HV = min(H, 4) heads of an edge
// (one 16-byte access at H >= 4) and LPE = H / HV neighbouring threads share an edge, so a wave instruction
// touches whole 128-byte lines (one lane per 32-byte record, as in the first version, touched every line twice
// and left the waves stalled on memory-instruction issue: SQ_WAIT_INST_ANY 55-73 %).
template <int H>
struct HeadSplit {
  static constexpr int HV = H >= 4 ? 4 : H;
  static constexpr int LPE = H / HV;
  static_assert(HV * LPE == H && (LPE & (LPE - 1)) == 0, "H must be 1, 2, 4, 8 or 16");
};

template <bool BLK, int LPE>
struct RowOwner {
  int64_t row, e0, e1;
  int tid, lane, wave;
  int sub;       // which HV-wide slice of an edge's heads this thread handles
  int etid;      // edge slot of this thread among the owner's threads
  int ethreads;  // edges the owner's threads cover per trip
  bool valid;
  __device__ __forceinline__ RowOwner(int64_t nv, const int64_t* rowptr, int heavy_thr,
                                      const uint32_t* row_list, const uint32_t* row_order) {
    lane = threadIdx.x & 63;
    wave = threadIdx.x >> 6;
    int nthreads;
    if constexpr (BLK) {
      row = row_list[row_order[blockIdx.x]];
      tid = threadIdx.x;
      nthreads = ROW_BLK_WAVES * 64;
      valid = true;
    } else {
      row = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
      tid = lane;
      nthreads = 64;
      valid = row < nv;
    }
    sub = tid % LPE;
    etid = tid / LPE;
    ethreads = nthreads / LPE;
    e0 = e1 = 0;
    if (valid) {
      e0 = rowptr[row];
      e1 = rowptr[row + 1];
      if (!BLK && heavy_thr > 0 && e1 - e0 > (int64_t)heavy_thr) valid = false;
    }
  }
};

// reductions over the lanes of a wave that handle the SAME head slice (lane % LPE equal)
template <int LPE>
__device__ __forceinline__ float slice_sum(float v) {
#pragma unroll
  for (int o = 32; o >= LPE; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int LPE>
__device__ __forceinline__ float slice_max(float v) {
#pragma unroll
  for (int o = 32; o >= LPE; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// sum over the row owner's threads of one head slice; lds: [ROW_BLK_WAVES][LPE][HV] floats (BLK only).  Fixed order.
template <int HV, int LPE, bool BLK>
__device__ __forceinline__ void owner_sum(HeadVec<HV>& v, int wave, int lane, int sub, float* lds) {
#pragma unroll
  for (int h = 0; h < HV; ++h) v.v[h] = slice_sum<LPE>(v.v[h]);
  if constexpr (BLK) {
    __syncthreads();  // lds may still be read from a previous reduction
    if (lane < LPE) {  // (lane == sub here)
#pragma unroll
      for (int h = 0; h < HV; ++h) lds[(wave * LPE + sub) * HV + h] = v.v[h];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < HV; ++h) {
      float t = lds[sub * HV + h];
      for (int w = 1; w < ROW_BLK_WAVES; ++w) t += lds[(w * LPE + sub) * HV + h];
      v.v[h] = t;
    }
  }
}

// (m, d) = (running maximum, sum of exp(s - m)) per thread -> the row's (M, D) of the thread's head slice
template <int HV, int LPE, bool BLK>
__device__ __forceinline__ void owner_softmax_stats(HeadVec<HV>& m, HeadVec<HV>& d, int wave, int lane, int sub,
                                                    float* lds) {
#pragma unroll
  for (int h = 0; h < HV; ++h) {
    const float mw = slice_max<LPE>(m.v[h]);
    const float scaled = (m.v[h] == -INFINITY) ? 0.f : d.v[h] * expf(m.v[h] - mw);
    d.v[h] = slice_sum<LPE>(scaled);
    m.v[h] = mw;
  }
  if constexpr (BLK) {
    __syncthreads();
    if (lane < LPE) {
#pragma unroll
      for (int h = 0; h < HV; ++h) {
        lds[((wave * LPE + sub) * HV + h) * 2] = m.v[h];
        lds[((wave * LPE + sub) * HV + h) * 2 + 1] = d.v[h];
      }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < HV; ++h) {
      float M = -INFINITY;
      for (int w = 0; w < ROW_BLK_WAVES; ++w) M = fmaxf(M, lds[((w * LPE + sub) * HV + h) * 2]);
      float D = 0.f;
      for (int w = 0; w < ROW_BLK_WAVES; ++w) {
        const float mw = lds[((w * LPE + sub) * HV + h) * 2];
        if (mw != -INFINITY) D += lds[((w * LPE + sub) * HV + h) * 2 + 1] * expf(mw - M);
      }
      m.v[h] = M;
      d.v[h] = D;
    }
  }
}

// temp = sl[i] + sr[col]; s = leaky_relu(temp); norm = softmax_row(s)   (gat_aggregator.cpp:64-77).
// Rows that fit one edge per thread group stay in registers; longer rows take two passes: an online
// (max, sum) pass that writes temp, then norm = exp(s - M) / D from the re-read temp.  132 B per edge
// at H = 8 (4 col + 32 gathered + 32 temp + 32 re-read + 32 norm); `scores` is optional (+32 B).
template <int H, bool BLK>
__global__ __launch_bounds__(BLK ? ROW_BLK_WAVES * 64 : 256) void edge_softmax_v2_kernel(
    int64_t nv, const int64_t* rowptr, const uint32_t* col, const float* sl, const float* sr, float eps,
    float* temp, float* scores, float* norm, int heavy_thr, const uint32_t* row_list, const uint32_t* row_order) {
  constexpr int HV = HeadSplit<H>::HV, LPE = HeadSplit<H>::LPE;
  __shared__ float lds[BLK ? ROW_BLK_WAVES * H * 2 : 1];
  const RowOwner<BLK, LPE> o(nv, rowptr, heavy_thr, row_list, row_order);
  if (!o.valid || o.e0 == o.e1) return;
  const int hb = o.sub * HV;  // first head of this thread's slice
  HeadVec<HV> ssrc, m, d;
  ssrc.load(sl + o.row * H + hb);
  if (!BLK && o.e1 - o.e0 <= 64 / LPE) {
    const int64_t e = o.e0 + o.etid;
    const bool ok = e < o.e1;
    HeadVec<HV> t, s;
    t.load(sr + (int64_t)(ok ? col[e] : 0u) * H + hb);
#pragma unroll
    for (int h = 0; h < HV; ++h) {
      t.v[h] = ssrc.v[h] + t.v[h];
      s.v[h] = ok ? (t.v[h] > 0.0f ? t.v[h] : eps * t.v[h]) : -INFINITY;
      const float mx = slice_max<LPE>(s.v[h]);
      const float ex = ok ? expf(s.v[h] - mx) : 0.f;
      const float den = slice_sum<LPE>(ex);
      m.v[h] = ex / den;
    }
    if (ok) {
      if (temp) t.store(temp + e * H + hb);
      if (scores) s.store(scores + e * H + hb);
      m.store(norm + e * H + hb);
    }
    return;
  }
#pragma unroll
  for (int h = 0; h < HV; ++h) { m.v[h] = -INFINITY; d.v[h] = 0.f; }
  // EU edges per thread per trip: all column ids, then all gathers, then the arithmetic
  constexpr int EU = 4;
  for (int64_t e = o.e0 + o.etid; e < o.e1; e += (int64_t)EU * o.ethreads) {
    uint32_t c[EU];
    HeadVec<HV> t[EU];
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int64_t eu = e + (int64_t)u * o.ethreads;
      c[u] = eu < o.e1 ? col[eu] : 0u;
    }
#pragma unroll
    for (int u = 0; u < EU; ++u) t[u].load(sr + (int64_t)c[u] * H + hb);
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int64_t eu = e + (int64_t)u * o.ethreads;
      if (eu < o.e1) {
        HeadVec<HV> s;
#pragma unroll
        for (int h = 0; h < HV; ++h) {
          t[u].v[h] = ssrc.v[h] + t[u].v[h];
          s.v[h] = t[u].v[h] > 0.0f ? t[u].v[h] : eps * t[u].v[h];
          // online softmax statistics with one expf: ex = exp(-|s - m|)
          const bool up = s.v[h] > m.v[h];
          const float ex = __expf(up ? m.v[h] - s.v[h] : s.v[h] - m.v[h]);
          d.v[h] = up ? d.v[h] * ex + 1.0f : d.v[h] + ex;
          m.v[h] = up ? s.v[h] : m.v[h];
        }
        if (temp) t[u].store(temp + eu * H + hb);
        if (scores) s.store(scores + eu * H + hb);
      }
    }
  }
  owner_softmax_stats<HV, LPE, BLK>(m, d, o.wave, o.lane, o.sub, lds);
#pragma unroll
  for (int h = 0; h < HV; ++h) d.v[h] = 1.0f / d.v[h];
  for (int64_t e = o.e0 + o.etid; e < o.e1; e += (int64_t)EU * o.ethreads) {
    HeadVec<HV> t[EU];
    if (temp) {  // each thread re-reads only its own writes
#pragma unroll
      for (int u = 0; u < EU; ++u) {
        const int64_t eu = e + (int64_t)u * o.ethreads;
        t[u].load(temp + (eu < o.e1 ? eu : o.e0) * H + hb);
      }
    } else {
      // no temp array asked for: the pre-activation score is formed again from the per-vertex dots (4 + 4H bytes
      // per edge out of the caches instead of 4H written and 4H read back through HBM); same sum, same bits
      uint32_t c[EU];
#pragma unroll
      for (int u = 0; u < EU; ++u) {
        const int64_t eu = e + (int64_t)u * o.ethreads;
        c[u] = col[eu < o.e1 ? eu : o.e0];
      }
#pragma unroll
      for (int u = 0; u < EU; ++u) t[u].load(sr + (int64_t)c[u] * H + hb);
#pragma unroll
      for (int u = 0; u < EU; ++u) {
#pragma unroll
        for (int h = 0; h < HV; ++h) t[u].v[h] = ssrc.v[h] + t[u].v[h];
      }
    }
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int64_t eu = e + (int64_t)u * o.ethreads;
      if (eu < o.e1) {
#pragma unroll
        for (int h = 0; h < HV; ++h) {
          const float sv = t[u].v[h] > 0.0f ? t[u].v[h] : eps * t[u].v[h];
          t[u].v[h] = __expf(sv - m.v[h]) * d.v[h];  // d holds 1/D here
        }
        t[u].store(norm + eu * H + hb);
      }
    }
  }
}

// softmax backward (math_functions.cpp:496-514, closed form of the :497-504 branch) + leaky-relu'
// (gat_aggregator.cpp:145): ds = p(1-p)dp - (dot - p dp) p with dot = sum_e p dp, g = ds * lrelu'(temp).
// Writes g into gbuf, the row sum of g into rs, ds into scores when asked.  DOT = true: the row's dot comes
// from the caller (rowdot[i,h] = <grad_i, forward output_i> on slice h -- the same sum regrouped by vertex),
// which makes this ONE pass over the edge arrays.
// RE = true: no temp array; the sign of the pre-activation score comes from sl[i] + sr[col] formed again.
template <int H, bool BLK, bool DOT, bool RE>
__global__ __launch_bounds__(BLK ? ROW_BLK_WAVES * 64 : 256) void softmax_bwd_v2_kernel(
    int64_t nv, const int64_t* rowptr, const float* p, const float* dp, const float* temp, float eps,
    const float* rowdot, float* scores, float* gbuf, int pack, float* rs, int heavy_thr,
    const uint32_t* row_list, const uint32_t* row_order, const uint32_t* col, const float* sl, const float* sr) {
  constexpr int HV = HeadSplit<H>::HV, LPE = HeadSplit<H>::LPE;
  __shared__ float lds[BLK ? ROW_BLK_WAVES * H : 1];
  const RowOwner<BLK, LPE> o(nv, rowptr, heavy_thr, row_list, row_order);
  if (!o.valid) return;
  const int hb = o.sub * HV;
  HeadVec<HV> dot, gs;
#pragma unroll
  for (int h = 0; h < HV; ++h) { dot.v[h] = 0.f; gs.v[h] = 0.f; }
  if constexpr (DOT) {
    dot.load(rowdot + o.row * H + hb);
  } else {
    for (int64_t e = o.e0 + o.etid; e < o.e1; e += o.ethreads) {
      HeadVec<HV> a, b;
      a.load(p + e * H + hb);
      b.load(dp + e * H + hb);
#pragma unroll
      for (int h = 0; h < HV; ++h) dot.v[h] += a.v[h] * b.v[h];
    }
    owner_sum<HV, LPE, BLK>(dot, o.wave, o.lane, o.sub, lds);
  }
  constexpr int EU = 4;
  HeadVec<HV> ssrc;
  if constexpr (RE) ssrc.load(sl + o.row * H + hb);
  for (int64_t e = o.e0 + o.etid; e < o.e1; e += (int64_t)EU * o.ethreads) {
    HeadVec<HV> a[EU], b[EU], t[EU];
    if constexpr (RE) {
      uint32_t c[EU];
#pragma unroll
      for (int u = 0; u < EU; ++u) {
        const int64_t eu = e + (int64_t)u * o.ethreads;
        c[u] = col[eu < o.e1 ? eu : o.e0];
      }
#pragma unroll
      for (int u = 0; u < EU; ++u) t[u].load(sr + (int64_t)c[u] * H + hb);
    }
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int64_t eu = e + (int64_t)u * o.ethreads;
      const int64_t es = eu < o.e1 ? eu : o.e0;
      a[u].load(p + es * H + hb);
      b[u].load(dp + es * H + hb);
      if constexpr (!RE) t[u].load(temp + es * H + hb);
    }
    if constexpr (RE) {
#pragma unroll
      for (int u = 0; u < EU; ++u) {
#pragma unroll
        for (int h = 0; h < HV; ++h) t[u].v[h] = ssrc.v[h] + t[u].v[h];
      }
    }
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int64_t eu = e + (int64_t)u * o.ethreads;
      if (eu < o.e1) {
        HeadVec<HV> ds, ge;
#pragma unroll
        for (int h = 0; h < HV; ++h) {
          const float x = a[u].v[h] * (1.0f - a[u].v[h]) * b[u].v[h];
          ds.v[h] = x - (dot.v[h] - a[u].v[h] * b[u].v[h]) * a[u].v[h];
          ge.v[h] = ds.v[h] * (t[u].v[h] > 0.0f ? 1.0f : eps);
          gs.v[h] += ge.v[h];
        }
        if (scores) ds.store(scores + eu * H + hb);
        if (pack) {  // (g, p) side by side: the column-sum pass fetches both with one random access
          ge.store(gbuf + eu * 2 * H + hb);
          a[u].store(gbuf + eu * 2 * H + H + hb);
        } else {
          ge.store(gbuf + eu * H + hb);
        }
      }
    }
  }
  owner_sum<HV, LPE, BLK>(gs, o.wave, o.lane, o.sub, lds);
  if (o.tid < LPE) gs.store(rs + o.row * H + hb);
}

// cs[v] = sum_{e in row v} g[rev[e]]  == column sum of g (structurally symmetric graph); optionally also
// pT[e] = p[rev[e]] (symmetric_csr_transpose of the attention, gat_aggregator.cpp:172-175); gbuf then holds
// (g, p) records written by softmax_bwd_v2_kernel
template <int H, bool BLK>
__global__ __launch_bounds__(BLK ? ROW_BLK_WAVES * 64 : 256) void colsum_v2_kernel(
    int64_t nv, const int64_t* rowptr, const uint32_t* rev, const float* gbuf, float* cs,
    float* pT, int heavy_thr, const uint32_t* row_list, const uint32_t* row_order) {
  constexpr int HV = HeadSplit<H>::HV, LPE = HeadSplit<H>::LPE;
  __shared__ float lds[BLK ? ROW_BLK_WAVES * H : 1];
  const RowOwner<BLK, LPE> o(nv, rowptr, heavy_thr, row_list, row_order);
  if (!o.valid) return;
  const int hb = o.sub * HV;
  HeadVec<HV> s;
#pragma unroll
  for (int h = 0; h < HV; ++h) s.v[h] = 0.f;
  constexpr int EU = 4;
  const int rec = (pT ? 2 : 1) * H;  // floats per edge record in gbuf
  for (int64_t e = o.e0 + o.etid; e < o.e1; e += (int64_t)EU * o.ethreads) {
    int64_t r[EU];
    HeadVec<HV> g[EU];
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int64_t eu = e + (int64_t)u * o.ethreads;
      r[u] = eu < o.e1 ? (int64_t)rev[eu] : -1;
    }
#pragma unroll
    for (int u = 0; u < EU; ++u) g[u].load(gbuf + (r[u] < 0 ? 0 : r[u]) * rec + hb);
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      if (r[u] >= 0) {
#pragma unroll
        for (int h = 0; h < HV; ++h) s.v[h] += g[u].v[h];
      }
    }
    if (pT) {  // the transposed attention for the gradient aggregation, while rev[e] is at hand
#pragma unroll
      for (int u = 0; u < EU; ++u) g[u].load(gbuf + (r[u] < 0 ? 0 : r[u]) * rec + H + hb);  // same line as g
#pragma unroll
      for (int u = 0; u < EU; ++u)
        if (r[u] >= 0) g[u].store(pT + (e + (int64_t)u * o.ethreads) * H + hb);
    }
  }
  owner_sum<HV, LPE, BLK>(s, o.wave, o.lane, o.sub, lds);
  if (o.tid < LPE) s.store(cs + o.row * H + hb);
}

// The same column sums over the graph's ordered 64-edge chunk list (gaib_graph_ensure_chunks): a wave takes one chunk,
// fetches the (g, p) records of its reverse edges, writes the chunk's piece of pT and one partial sum per head; a second
// kernel adds a row's partials in row order.  Row by row, the 8192 rows in flight each sweep the whole 7 GB record array
// (the reverse edge of (v -> c) sits in row c's segment); chunk by chunk in column order, everything in flight points
// into the segments of one window of rows.
template <int H>
__global__ __launch_bounds__(256) void colsum_chunk_kernel(int64_t n_chunks, const uint32_t* chunk_row,
                                                           const uint32_t* chunk_ebase, const uint32_t* chunk_start,
                                                           const int64_t* rowptr, const uint32_t* rev, const float* gbuf,
                                                           float* partial, float* pT) {
  constexpr int HV = HeadSplit<H>::HV, LPE = HeadSplit<H>::LPE;
  constexpr int EPP = 64 / LPE;  // edges per pass; a 64-edge chunk takes LPE passes
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const int sub = lane % LPE, etid = lane / LPE, hb = sub * HV;
  const int64_t row = chunk_row[c];
  const int64_t eb = chunk_ebase[c];
  const int64_t rem = rowptr[row + 1] - eb;
  const int n = rem < 64 ? (int)rem : 64;
  const int rec = (pT ? 2 : 1) * H;
  int64_t r[LPE];
  HeadVec<HV> g[LPE], s;
#pragma unroll
  for (int h = 0; h < HV; ++h) s.v[h] = 0.f;
#pragma unroll
  for (int ps = 0; ps < LPE; ++ps) {
    const int ei = ps * EPP + etid;
    r[ps] = ei < n ? (int64_t)rev[eb + ei] : -1;
  }
#pragma unroll
  for (int ps = 0; ps < LPE; ++ps) g[ps].load(gbuf + (r[ps] < 0 ? 0 : r[ps]) * rec + hb);
#pragma unroll
  for (int ps = 0; ps < LPE; ++ps) {
    if (r[ps] >= 0) {
#pragma unroll
      for (int h = 0; h < HV; ++h) s.v[h] += g[ps].v[h];
    }
  }
  if (pT) {
#pragma unroll
    for (int ps = 0; ps < LPE; ++ps) g[ps].load(gbuf + (r[ps] < 0 ? 0 : r[ps]) * rec + H + hb);  // same line as g
#pragma unroll
    for (int ps = 0; ps < LPE; ++ps)
      if (r[ps] >= 0) g[ps].store(pT + (eb + ps * EPP + etid) * H + hb);
  }
#pragma unroll
  for (int h = 0; h < HV; ++h) s.v[h] = slice_sum<LPE>(s.v[h]);
  const int64_t slot = (int64_t)chunk_start[row] + (eb - rowptr[row]) / 64;
  if (lane < LPE) s.store(partial + slot * H + hb);
}

// cs[v, h] = sum of row v's chunk partials, in row order
__global__ void colsum_reduce_kernel(int64_t nv, int H, const uint32_t* chunk_start, const float* partial, float* cs) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nv * H) return;
  const int64_t v = t / H;
  const int h = (int)(t - v * H);
  float s = 0.f;
  for (int64_t k = chunk_start[v]; k < chunk_start[v + 1]; ++k) s += partial[k * H + h];
  cs[t] = s;
}

// sign(t_e) of every (edge, head) pre-activation score EXACTLY as the one-sweep kernels above form it (the same FMA
// chains, the same DPP sums, the same add): leaky_relu' jumps at t = 0, and a score within rounding of zero takes either
// slope in two correct fp32 evaluations -- a test that wants to compare ARITHMETIC with an fp64 evaluation of the alpha
// gradients imposes these signs on it (the way the relu mask of the oracle's forward output is imposed on the GPU's
// backward).  Test / diagnostic entry point (gaib_gat_score_signs); not on the training path.
// (a diagnostic kernel: where hipcc does not unroll its 16-/32-step loop for some shape, the column id of step j comes through a
// switch instead of a constant DPP pattern -- slower, the same values; not worth failing the -Werror=pass-failed build over)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
template <int G, int H>
__global__ __launch_bounds__(256) void gat_score_sign_kernel(int64_t n_chunks, const uint32_t* chunk_row, const uint32_t* chunk_ebase,
                                                             const int64_t* rowptr, const uint32_t* col, int len, const float* feat,
                                                             const float* alpha_l, const float* alpha_r, uint8_t* sign_out) {
  constexpr int LH = G / H;
  using CL = ChunkLanes<G>;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const int sl = lane & (G - 1);
  const int64_t row = chunk_row[c];
  const int64_t eb = chunk_ebase[c];
  const int64_t rem = rowptr[row + 1] - eb;
  const int n = rem < 64 ? (int)rem : 64;
  const int my_e = CL::held_edge(lane, 0), my_e1 = CL::held_edge(lane, 1);
  const uint32_t cl = col[eb + (my_e < n ? my_e : 0)];
  uint32_t cl1 = 0;
  if constexpr (G == 32) cl1 = col[eb + (my_e1 < n ? my_e1 : 0)];
  const int coff = sl * 4;
  const int head = sl / LH;
  const f4 hi = *reinterpret_cast<const f4*>(feat + row * (int64_t)len + coff);
  const f4 al4 = *reinterpret_cast<const f4*>(alpha_l + coff);
  const f4 ar4 = *reinterpret_cast<const f4*>(alpha_r + coff);
  auto d4 = [](const f4& a, const f4& b) {
    return __builtin_fmaf(a[3], b[3], __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0])));
  };
  const float sl_i = lanes_sum_w<LH>(d4(al4, hi));
#pragma unroll
  for (int j = 0; j < G; ++j) {
    if (j * CL::NG >= n) break;
    const uint32_t cj = (uint32_t)CL::step_value((int)cl, (int)cl1, lane, j);
    const f4 xh = *reinterpret_cast<const f4*>(feat + (int64_t)cj * len + coff);
    const float sr_c = lanes_sum_w<LH>(d4(ar4, xh));
    const float t_e = sl_i + sr_c;
    const int ei = CL::step_edge(lane, j);
    if (ei < n && (sl & (LH - 1)) == 0) sign_out[(eb + ei) * H + head] = t_e > 0.0f ? 1 : 0;
  }
}
#pragma clang diagnostic pop

// the row-owner kernels: gat_row_waves (1, 2 or 4) one-wave rows per workgroup
inline unsigned rowgrid_w(const gaib_ctx* ctx, int64_t nv) { return (unsigned)cdiv64(nv > 0 ? nv : 1, ctx->gat_row_waves); }

template <int H>
int launch_edge_softmax(gaib_ctx* ctx, gaib_graph* g, const float* sl, const float* sr, float eps, float* temp,
                        float* scores, float* norm) {
  GAIB_TRY(gaib_graph_ensure_heavy(ctx, g, ctx->spmm_heavy_threshold));
  const uint32_t* rl = g->heavy_rows;
  const uint32_t* ro = g->heavy_rows ? g->heavy_rows + g->n_heavy : nullptr;
  const int thr = g->n_heavy > 0 ? g->heavy_thr : 0;
  if (g->n_heavy > 0) {  // long rows first: their tail hides under the light launch
    edge_softmax_v2_kernel<H, true><<<(unsigned)g->n_heavy, ROW_BLK_WAVES * 64, 0, ctx->stream>>>(
        g->nv, g->rowptr, g->colidx, sl, sr, eps, temp, scores, norm, thr, rl, ro);
    GAIB_LAUNCH_CHECK();
  }
  edge_softmax_v2_kernel<H, false><<<rowgrid_w(ctx, g->nv), ctx->gat_row_waves * 64, 0, ctx->stream>>>(
      g->nv, g->rowptr, g->colidx, sl, sr, eps, temp, scores, norm, thr, rl, ro);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

template <int H>
int launch_softmax_bwd(gaib_ctx* ctx, gaib_graph* g, const float* p, const float* dp, const float* temp, float eps,
                       const float* rowdot, float* scores, float* gbuf, float* rs, float* cs, float* pT,
                       const float* sl, const float* sr, float* colsum_partial) {
  GAIB_TRY(gaib_graph_ensure_heavy(ctx, g, ctx->spmm_heavy_threshold));
  const uint32_t* rl = g->heavy_rows;
  const uint32_t* ro = g->heavy_rows ? g->heavy_rows + g->n_heavy : nullptr;
  const int thr = g->n_heavy > 0 ? g->heavy_thr : 0;
  const unsigned nh = (unsigned)g->n_heavy, blk = ROW_BLK_WAVES * 64;
  const unsigned lg = rowgrid_w(ctx, g->nv), lb = (unsigned)ctx->gat_row_waves * 64;
#define GAIB_SBW_LAUNCH(DOT, RE)                                                                                   \
  do {                                                                                                             \
    if (nh)                                                                                                        \
      softmax_bwd_v2_kernel<H, true, DOT, RE><<<nh, blk, 0, ctx->stream>>>(                                        \
          g->nv, g->rowptr, p, dp, temp, eps, rowdot, scores, gbuf, pT ? 1 : 0, rs, thr, rl, ro, g->colidx, sl, sr); \
    softmax_bwd_v2_kernel<H, false, DOT, RE><<<lg, lb, 0, ctx->stream>>>(                                          \
        g->nv, g->rowptr, p, dp, temp, eps, rowdot, scores, gbuf, pT ? 1 : 0, rs, thr, rl, ro, g->colidx, sl, sr);   \
  } while (0)
  if (rowdot) {
    if (temp) GAIB_SBW_LAUNCH(true, false);
    else GAIB_SBW_LAUNCH(true, true);
  } else {
    if (temp) GAIB_SBW_LAUNCH(false, false);
    else GAIB_SBW_LAUNCH(false, true);
  }
#undef GAIB_SBW_LAUNCH
  GAIB_LAUNCH_CHECK();
  if (colsum_partial) {  // dense graphs: chunk by chunk in column order (the caller reserved the partials)
    colsum_chunk_kernel<H><<<(unsigned)cdiv64(g->n_chunks > 0 ? g->n_chunks : 1, 4), 256, 0, ctx->stream>>>(
        g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->rev, gbuf, colsum_partial, pT);
    GAIB_LAUNCH_CHECK();
    colsum_reduce_kernel<<<(unsigned)cdiv64(g->nv * H, 256), 256, 0, ctx->stream>>>(g->nv, H, g->chunk_start,
                                                                                  colsum_partial, cs);
    GAIB_LAUNCH_CHECK();
    return GAIB_OK;
  }
  if (nh) colsum_v2_kernel<H, true><<<nh, blk, 0, ctx->stream>>>(g->nv, g->rowptr, g->rev, gbuf, cs, pT, thr, rl, ro);
  colsum_v2_kernel<H, false><<<lg, lb, 0, ctx->stream>>>(g->nv, g->rowptr, g->rev, gbuf, cs, pT, thr, rl, ro);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

}  // namespace

extern "C" int gaib_gat_scores_mh(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h,
                                  const float* d_alpha_l, const float* d_alpha_r, float epsilon,
                                  float* d_temp_scores, float* d_scores, float* d_norm_scores) {
  GAIB_CHECK(ctx && g, "gaib_gat_scores: NULL ctx/graph");
  GAIB_TRY(check_heads("gaib_gat_scores", len, heads));
  if (g->nv == 0) return GAIB_OK;
  GAIB_CHECK(d_h && d_alpha_l && d_alpha_r && d_norm_scores, "gaib_gat_scores: NULL pointer");
  // rectangular graphs (a rank's rows over [owned | halo] columns): d_h is the COLUMN table [nc x len] whose first nv
  // rows are the rows' own vectors; the per-vertex dots are taken over all nc rows
  const int64_t nt = g->nc > g->nv ? g->nc : g->nv;
  GAIB_HIP(hipSetDevice(ctx->device));
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * 2 * (size_t)nt * heads));
  float* sl = (float*)ctx->ws;
  float* sr = sl + nt * heads;
  {
    ProfScope ps(ctx, "gat_vertex_dots", (double)nt * (4.0 * len + 8.0 * heads), 4.0 * (double)nt * len);
    vertex_dots_kernel<<<rowgrid(nt), 256, 0, ctx->stream>>>(nt, len, heads, d_h, d_alpha_l, d_alpha_r, sl, sr);
  }
  GAIB_LAUNCH_CHECK();
  {
    ProfScope ps(ctx, "gat_edge_softmax", (double)g->ne * (4.0 + 4.0 * heads + 2 * 4.0 * heads) + (double)g->nv * 8.0 * heads);
    const bool al16 = (((uintptr_t)d_temp_scores | (uintptr_t)d_scores | (uintptr_t)d_norm_scores) & 15) == 0;
    int rc = GAIB_OK;
    if (heads == 1) rc = launch_edge_softmax<1>(ctx, g, sl, sr, epsilon, d_temp_scores, d_scores, d_norm_scores);
    else if (heads == 2) rc = launch_edge_softmax<2>(ctx, g, sl, sr, epsilon, d_temp_scores, d_scores, d_norm_scores);
    else if (heads == 4 && al16) rc = launch_edge_softmax<4>(ctx, g, sl, sr, epsilon, d_temp_scores, d_scores, d_norm_scores);
    else if (heads == 8 && al16) rc = launch_edge_softmax<8>(ctx, g, sl, sr, epsilon, d_temp_scores, d_scores, d_norm_scores);
    else if (heads == 16 && al16) rc = launch_edge_softmax<16>(ctx, g, sl, sr, epsilon, d_temp_scores, d_scores, d_norm_scores);
    else {
      GAIB_CHECK(d_scores && d_temp_scores, "gaib_gat_scores: this head count needs d_temp_scores and d_scores");
      edge_softmax_kernel<<<rowgrid(g->nv), 256, 0, ctx->stream>>>(
          g->nv, heads, g->rowptr, g->colidx, sl, sr, epsilon, d_temp_scores, d_scores, d_norm_scores);
    }
    if (rc != GAIB_OK) return rc;
  }
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_gat_scores(gaib_ctx* ctx, gaib_graph* g, int len, const float* d_h,
                               const float* d_alpha_l, const float* d_alpha_r, float epsilon,
                               float* d_temp_scores, float* d_scores, float* d_norm_scores) {
  return gaib_gat_scores_mh(ctx, g, len, 1, d_h, d_alpha_l, d_alpha_r, epsilon, d_temp_scores, d_scores,
                            d_norm_scores);
}

extern "C" int gaib_sddmm_mh(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_grad,
                             const float* d_feat, float* d_out_e) {
  GAIB_CHECK(ctx && g, "gaib_sddmm: NULL ctx/graph");
  GAIB_TRY(check_heads("gaib_sddmm", len, heads));
  if (g->nv == 0 || g->ne == 0) return GAIB_OK;
  GAIB_CHECK(d_grad && d_feat && d_out_e, "gaib_sddmm: NULL pointer");
  GAIB_HIP(hipSetDevice(ctx->device));
  const int dh = len / heads;
  const int lh = dh / 4;  // lanes per head in the chunk kernels
  const bool vec_ok = (len % 4 == 0) && len <= 256 && ((((uintptr_t)d_grad | (uintptr_t)d_feat) & 15) == 0) &&
                      ctx->gat_fast && (heads == 1 || (dh % 4 == 0 && (lh & (lh - 1)) == 0));
  if (vec_ok) {
    GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
    ProfScope ps(ctx, "gat_sddmm", (double)g->ne * (4.0 + 4.0 * len + 4.0 * heads) + (double)g->nv * 4.0 * len, 2.0 * (double)g->ne * len);
    const unsigned grid = (unsigned)cdiv64(g->n_chunks > 0 ? g->n_chunks : 1, 4);
#define GAIB_SDDMM(G, U, LH)                                                                            \
  sddmm_chunk_kernel<G, U, LH><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, \
                                                              g->rowptr, g->colidx, len, heads, d_grad, d_feat, d_out_e)
    if (heads == 1) {
      if (len <= 4) GAIB_SDDMM(1, 1, 1);
      else if (len <= 8) GAIB_SDDMM(2, 2, 2);
      else if (len <= 16) GAIB_SDDMM(4, 4, 4);
      else if (len <= 32) GAIB_SDDMM(8, 8, 8);
      else if (len <= 64) GAIB_SDDMM(16, 8, 16);
      else if (len <= 128) GAIB_SDDMM(32, 8, 32);
      else GAIB_SDDMM(64, 8, 64);
    } else {
      // G = lanes per edge (power of two covering len/4), LH = lanes per head (< G since heads > 1)
      if (len <= 8) GAIB_SDDMM(2, 2, 1);
      else if (len <= 16) { if (lh == 1) GAIB_SDDMM(4, 4, 1); else GAIB_SDDMM(4, 4, 2); }
      else if (len <= 32) { if (lh == 1) GAIB_SDDMM(8, 8, 1); else if (lh == 2) GAIB_SDDMM(8, 8, 2); else GAIB_SDDMM(8, 8, 4); }
      else if (len <= 64) {
        if (lh == 1) GAIB_SDDMM(16, 8, 1); else if (lh == 2) GAIB_SDDMM(16, 8, 2);
        else if (lh == 4) GAIB_SDDMM(16, 8, 4); else GAIB_SDDMM(16, 8, 8);
      } else if (len <= 128) {
        if (lh == 1) GAIB_SDDMM(32, 8, 1); else if (lh == 2) GAIB_SDDMM(32, 8, 2);
        else if (lh == 4) GAIB_SDDMM(32, 8, 4); else if (lh == 8) GAIB_SDDMM(32, 8, 8); else GAIB_SDDMM(32, 8, 16);
      } else {
        if (lh == 1) GAIB_SDDMM(64, 8, 1); else if (lh == 2) GAIB_SDDMM(64, 8, 2);
        else if (lh == 4) GAIB_SDDMM(64, 8, 4); else if (lh == 8) GAIB_SDDMM(64, 8, 8);
        else if (lh == 16) GAIB_SDDMM(64, 8, 16); else GAIB_SDDMM(64, 8, 32);
      }
    }
#undef GAIB_SDDMM
    GAIB_LAUNCH_CHECK();
    return GAIB_OK;
  }
  ProfScope ps(ctx, "gat_sddmm", (double)g->ne * (4.0 + 4.0 * len + 4.0 * heads) + (double)g->nv * 4.0 * len, 2.0 * (double)g->ne * len);
  sddmm_generic_kernel<<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, heads, g->rowptr, g->colidx, len,
                                                               d_grad, d_feat, d_out_e);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_sddmm(gaib_ctx* ctx, gaib_graph* g, int len, const float* d_grad,
                          const float* d_feat, float* d_out_e) {
  return gaib_sddmm_mh(ctx, g, len, 1, d_grad, d_feat, d_out_e);
}

// d_temp_scores == NULL: the sign of the pre-activation score is formed again from d_feat and (d_alpha_l, d_alpha_r)
static int softmax_bwd_alpha_impl(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat,
                                  const float* d_norm_scores, const float* d_norm_scores_grad,
                                  const float* d_temp_scores, const float* d_alpha_l, const float* d_alpha_r,
                                  float epsilon, float* d_scores, float* d_alpha_lgrad, float* d_alpha_rgrad,
                                  const float* d_grad_rows, const float* d_fwd_out_rows, float* d_norm_scores_t) {
  GAIB_CHECK(ctx && g, "gaib_gat_softmax_bwd_alpha: NULL ctx/graph");
  GAIB_TRY(check_heads("gaib_gat_softmax_bwd_alpha", len, heads));
  GAIB_CHECK(d_alpha_lgrad && d_alpha_rgrad, "gaib_gat_softmax_bwd_alpha: NULL alpha grad");
  GAIB_HIP(hipSetDevice(ctx->device));
  if (g->nv == 0) return GAIB_OK;
  GAIB_CHECK(d_feat && d_norm_scores && d_norm_scores_grad && (d_temp_scores || (d_alpha_l && d_alpha_r)),
             "gaib_gat_softmax_bwd_alpha: NULL pointer");
  GAIB_CHECK((d_grad_rows == nullptr) == (d_fwd_out_rows == nullptr),
             "gaib_gat_softmax_bwd_alpha: d_grad_rows and d_fwd_out_rows go together");
  GAIB_TRY(gaib_graph_ensure_rev(ctx, g));
  const int nblocks = gat_alpha_blocks(g->nv);
  const size_t n_g = up4((size_t)g->ne * heads * (d_norm_scores_t ? 2 : 1)), n_v = up4((size_t)g->nv * heads);
  // graphs with a quarter of their edges in heavy rows, 1-2 heads: the column sums go chunk by chunk (reddit shape: 2.86 -> 2.67 ms single-head; at 8 heads
  // the 64-byte records gain nothing, 7.10 vs 7.11 ms).  gat_chunk_colsum: -1 = that rule, 0 never, 1 always.
  GAIB_TRY(gaib_graph_ensure_heavy(ctx, g, ctx->spmm_heavy_threshold));
  const bool v2_heads = heads == 1 || heads == 2 || heads == 4 || heads == 8 || heads == 16;
  const bool chunk_cs = v2_heads && g->ne > 0 &&
                        (ctx->gat_chunk_colsum == 1 ||
                         (ctx->gat_chunk_colsum < 0 && heads <= 2 && g->n_heavy > 0 && 4 * g->heavy_edges >= g->ne));
  if (chunk_cs) GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  const size_t n_p = chunk_cs ? up4((size_t)g->n_chunks * heads) : 0;
  const size_t ws_floats = n_g + 5 * n_v + n_p + (size_t)nblocks * 2 * len;
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * ws_floats));
  float* gbuf = (float*)ctx->ws;
  float* rs = gbuf + n_g;
  float* cs = rs + n_v;
  float* rowdot = cs + n_v;
  float* sl = rowdot + n_v;
  float* sr = sl + n_v;
  float* cs_partial = sr + n_v;
  float* partial = cs_partial + n_p;
  ProfScope ps(ctx, "gat_softmax_bwd_alpha", (double)g->ne * (4.0 + 4.0 + 3 * 4.0 * heads) + (double)g->nv * (2 * 4.0 * len));
  if (!d_temp_scores) {
    vertex_dots_kernel<<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, d_feat, d_alpha_l, d_alpha_r, sl, sr);
    GAIB_LAUNCH_CHECK();
  }
  if (d_grad_rows) {
    rowdot_kernel<<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, d_grad_rows, d_fwd_out_rows, rowdot);
    GAIB_LAUNCH_CHECK();
  } else {
    rowdot = nullptr;
  }
  const bool al16 = (((uintptr_t)d_norm_scores | (uintptr_t)d_norm_scores_grad | (uintptr_t)d_temp_scores |
                      (uintptr_t)d_scores | (uintptr_t)gbuf | (uintptr_t)rs | (uintptr_t)cs |
                      (uintptr_t)d_norm_scores_t) & 15) == 0;
  int rc = GAIB_OK;
#define GAIB_SBW(HH) rc = launch_softmax_bwd<HH>(ctx, g, d_norm_scores, d_norm_scores_grad, d_temp_scores, epsilon, \
                                                 rowdot, d_scores, gbuf, rs, cs, d_norm_scores_t, sl, sr, \
                                                 chunk_cs ? cs_partial : nullptr)
  if (heads == 1) GAIB_SBW(1);
  else if (heads == 2) GAIB_SBW(2);
  else if (heads == 4 && al16) GAIB_SBW(4);
  else if (heads == 8 && al16) GAIB_SBW(8);
  else if (heads == 16 && al16) GAIB_SBW(16);
  else {
    GAIB_CHECK(d_scores && d_temp_scores, "gaib_gat_softmax_bwd_alpha: this head count needs d_temp_scores and d_scores");
    softmax_bwd_kernel<<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, heads, g->rowptr, d_norm_scores,
                                                                d_norm_scores_grad, d_temp_scores, epsilon,
                                                                d_scores, gbuf, rs);
    colsum_kernel<<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, heads, g->rowptr, g->rev, gbuf, cs);
    if (d_norm_scores_t) {
      GAIB_LAUNCH_CHECK();
      GAIB_TRY(gaib_edge_transpose_mh(ctx, g, heads, d_norm_scores, d_norm_scores_t));
    }
  }
#undef GAIB_SBW
  if (rc != GAIB_OK) return rc;
  GAIB_LAUNCH_CHECK();
  return launch_alpha_grads(ctx, g->nv, len, heads, d_feat, rs, cs, partial, d_alpha_lgrad, d_alpha_rgrad);
}

extern "C" int gaib_gat_score_signs(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h, const float* d_alpha_l,
                                    const float* d_alpha_r, uint8_t* d_sign_out) {
  GAIB_CHECK(ctx && g && d_h && d_alpha_l && d_alpha_r && d_sign_out, "gaib_gat_score_signs: NULL argument");
  GAIB_TRY(check_heads("gaib_gat_score_signs", len, heads));
  GAIB_CHECK(gat_fused_shape(len, heads),
             "gaib_gat_score_signs: the one-sweep kernels' shapes only (len 32, 64 or 128; 1, 2, 4, 8 or 16 heads of >= 4 columns)");
  GAIB_HIP(hipSetDevice(ctx->device));
  if (g->ne == 0) return GAIB_OK;
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  const unsigned grid = (unsigned)cdiv64(g->n_chunks, 4);
#define GAIB_SS(GG, HH)                                                                                                 \
  gat_score_sign_kernel<GG, HH><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->rowptr,     \
                                                               g->colidx, len, d_h, d_alpha_l, d_alpha_r, d_sign_out)
  GAIB_GAT_DISPATCH(GAIB_SS);
#undef GAIB_SS
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// ---- the pieces of GAT backward that work on RECTANGULAR graphs (a rank's share of a partition) ------
// On a partition the reverse edge of (i -> c) lives on the rank that owns c, so the reverse-edge permutation of the
// square path is replaced by the rank's TRANSPOSED local structure (rows = owned + halo vertices, columns = owned rows,
// built by the host with the edge permutation CSC position -> CSR edge id):
//   gaib_gat_softmax_bwd_rows  per-row softmax backward + leaky-relu': g_e and the row sums rs (no column side)
//   gaib_edge_gather_perm      out_e[k] = in_e[perm[k]]   (g and p in transposed order)
//   gaib_edge_rowsum           out[v] = sum over row v of an edge array   (column sums of g = row sums over the transpose)
//   gaib_gat_alpha_grads       alpha_l' = sum_v rs[v] x[v], alpha_r' = sum_v cs[v] x[v]   (fixed two-level reduction)
// and the transposed aggregation is gaib_spmm_mh on the transposed graph followed by gaib_halo_reduce.
extern "C" int gaib_gat_softmax_bwd_rows(gaib_ctx* ctx, gaib_graph* g, int heads, const float* d_norm_scores,
                                         const float* d_norm_scores_grad, const float* d_temp_scores, float epsilon,
                                         float* d_g_out, float* d_rs_out) {
  GAIB_CHECK(ctx && g, "gaib_gat_softmax_bwd_rows: NULL ctx/graph");
  GAIB_CHECK(heads >= 1, "gaib_gat_softmax_bwd_rows: heads must be >= 1");
  if (g->nv == 0) return GAIB_OK;  // (a rank without rows: its per-edge arrays may be NULL)
  GAIB_CHECK(d_norm_scores && d_norm_scores_grad && d_temp_scores && d_g_out && d_rs_out, "gaib_gat_softmax_bwd_rows: NULL argument");
  GAIB_HIP(hipSetDevice(ctx->device));
  const bool al16 = (((uintptr_t)d_norm_scores | (uintptr_t)d_norm_scores_grad | (uintptr_t)d_temp_scores |
                      (uintptr_t)d_g_out | (uintptr_t)d_rs_out) & 15) == 0;
  ProfScope ps(ctx, "gat_softmax_bwd_alpha", (double)g->ne * (4.0 + 4.0 + 3 * 4.0 * heads));
  GAIB_TRY(gaib_graph_ensure_heavy(ctx, g, ctx->spmm_heavy_threshold));
  const uint32_t* rl = g->heavy_rows;
  const uint32_t* ro = g->heavy_rows ? g->heavy_rows + g->n_heavy : nullptr;
  const int thr = g->n_heavy > 0 ? g->heavy_thr : 0;
  const unsigned nh = (unsigned)g->n_heavy, blk = ROW_BLK_WAVES * 64;
  const unsigned lg = rowgrid_w(ctx, g->nv), lb = (unsigned)ctx->gat_row_waves * 64;
#define GAIB_ROWS(HH)                                                                                                    \
  do {                                                                                                                   \
    if (nh)                                                                                                              \
      softmax_bwd_v2_kernel<HH, true, false, false><<<nh, blk, 0, ctx->stream>>>(                                        \
          g->nv, g->rowptr, d_norm_scores, d_norm_scores_grad, d_temp_scores, epsilon, nullptr, nullptr, d_g_out, 0,      \
          d_rs_out, thr, rl, ro, g->colidx, nullptr, nullptr);                                                           \
    softmax_bwd_v2_kernel<HH, false, false, false><<<lg, lb, 0, ctx->stream>>>(                                          \
        g->nv, g->rowptr, d_norm_scores, d_norm_scores_grad, d_temp_scores, epsilon, nullptr, nullptr, d_g_out, 0,        \
        d_rs_out, thr, rl, ro, g->colidx, nullptr, nullptr);                                                             \
  } while (0)
  if (heads == 1) GAIB_ROWS(1);
  else if (heads == 2) GAIB_ROWS(2);
  else if (heads == 4 && al16) GAIB_ROWS(4);
  else if (heads == 8 && al16) GAIB_ROWS(8);
  else if (heads == 16 && al16) GAIB_ROWS(16);
  else {
    // generic head counts: the kernel also writes ds; park it in the workspace
    GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (size_t)g->ne * heads));
    softmax_bwd_kernel<<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, heads, g->rowptr, d_norm_scores, d_norm_scores_grad,
                                                                d_temp_scores, epsilon, (float*)ctx->ws, d_g_out, d_rs_out);
  }
#undef GAIB_ROWS
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_edge_gather_perm(gaib_ctx* ctx, int64_t ne, int heads, const uint32_t* d_perm, const float* d_in_e,
                                     float* d_out_e) {
  GAIB_CHECK(ctx && heads >= 1 && ne >= 0, "gaib_edge_gather_perm: bad argument");
  if (ne == 0) return GAIB_OK;
  GAIB_CHECK(d_perm && d_in_e && d_out_e && d_in_e != d_out_e, "gaib_edge_gather_perm: NULL or aliased pointer");
  GAIB_HIP(hipSetDevice(ctx->device));
  edge_gather_kernel<<<(unsigned)cdiv64(ne * heads, 256), 256, 0, ctx->stream>>>(ne, heads, d_perm, d_in_e, d_out_e);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

__global__ __launch_bounds__(256) void edge_rowsum_kernel(int64_t nv, int H, const int64_t* rowptr, const float* in_e,
                                                          float* out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int lane = threadIdx.x & 63;
  const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
  for (int h = 0; h < H; ++h) {
    float s = 0.f;
    for (int64_t e = e0 + lane; e < e1; e += 64) s += in_e[e * H + h];
    s = wave_sum(s);
    if (lane == 0) out[row * H + h] = s;
  }
}

extern "C" int gaib_edge_rowsum(gaib_ctx* ctx, gaib_graph* g, int heads, const float* d_in_e, float* d_out_rows) {
  GAIB_CHECK(ctx && g && heads >= 1, "gaib_edge_rowsum: bad argument");
  if (g->nv == 0) return GAIB_OK;  // (a rank without rows: the arrays may be NULL)
  GAIB_CHECK(d_out_rows && (d_in_e || g->ne == 0), "gaib_edge_rowsum: NULL pointer");
  GAIB_HIP(hipSetDevice(ctx->device));
  edge_rowsum_kernel<<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, heads, g->rowptr, d_in_e, d_out_rows);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_gat_alpha_grads(gaib_ctx* ctx, int64_t nv, int len, int heads, const float* d_x, const float* d_rs,
                                    const float* d_cs, float* d_alpha_lgrad, float* d_alpha_rgrad) {
  GAIB_CHECK(ctx && d_alpha_lgrad && d_alpha_rgrad && nv >= 0, "gaib_gat_alpha_grads: bad argument");
  GAIB_TRY(check_heads("gaib_gat_alpha_grads", len, heads));
  GAIB_HIP(hipSetDevice(ctx->device));
  if (nv == 0) {  // no vertices (a rank without rows): both gradients are zero
    GAIB_HIP(hipMemsetAsync(d_alpha_lgrad, 0, sizeof(float) * len, ctx->stream));
    GAIB_HIP(hipMemsetAsync(d_alpha_rgrad, 0, sizeof(float) * len, ctx->stream));
    return GAIB_OK;
  }
  GAIB_CHECK(d_x && d_rs && d_cs, "gaib_gat_alpha_grads: NULL pointer");
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (size_t)gat_alpha_blocks(nv) * 2 * len));
  return launch_alpha_grads(ctx, nv, len, heads, d_x, d_rs, d_cs, (float*)ctx->ws, d_alpha_lgrad, d_alpha_rgrad);
}

extern "C" int gaib_gat_softmax_bwd_alpha_ex(gaib_ctx* ctx, gaib_graph* g, int len, int heads,
                                             const float* d_feat, const float* d_norm_scores,
                                             const float* d_norm_scores_grad,
                                             const float* d_temp_scores, float epsilon,
                                             float* d_scores, float* d_alpha_lgrad,
                                             float* d_alpha_rgrad, const float* d_grad_rows,
                                             const float* d_fwd_out_rows, float* d_norm_scores_t) {
  GAIB_CHECK(d_temp_scores, "gaib_gat_softmax_bwd_alpha: NULL pointer");
  return softmax_bwd_alpha_impl(ctx, g, len, heads, d_feat, d_norm_scores, d_norm_scores_grad, d_temp_scores, nullptr,
                                nullptr, epsilon, d_scores, d_alpha_lgrad, d_alpha_rgrad, d_grad_rows, d_fwd_out_rows,
                                d_norm_scores_t);
}

extern "C" int gaib_gat_softmax_bwd_alpha_re(gaib_ctx* ctx, gaib_graph* g, int len, int heads,
                                             const float* d_feat, const float* d_alpha_l, const float* d_alpha_r,
                                             const float* d_norm_scores, const float* d_norm_scores_grad,
                                             float epsilon, float* d_scores, float* d_alpha_lgrad,
                                             float* d_alpha_rgrad, const float* d_grad_rows,
                                             const float* d_fwd_out_rows, float* d_norm_scores_t) {
  GAIB_CHECK(d_alpha_l && d_alpha_r, "gaib_gat_softmax_bwd_alpha_re: NULL alpha");
  GAIB_CHECK(heads == 1 || heads == 2 || heads == 4 || heads == 8 || heads == 16,
             "gaib_gat_softmax_bwd_alpha_re: heads must be 1, 2, 4, 8 or 16");
  return softmax_bwd_alpha_impl(ctx, g, len, heads, d_feat, d_norm_scores, d_norm_scores_grad, nullptr, d_alpha_l,
                                d_alpha_r, epsilon, d_scores, d_alpha_lgrad, d_alpha_rgrad, d_grad_rows, d_fwd_out_rows,
                                d_norm_scores_t);
}

extern "C" int gaib_gat_softmax_bwd_alpha_mh(gaib_ctx* ctx, gaib_graph* g, int len, int heads,
                                             const float* d_feat, const float* d_norm_scores,
                                             const float* d_norm_scores_grad,
                                             const float* d_temp_scores, float epsilon,
                                             float* d_scores, float* d_alpha_lgrad,
                                             float* d_alpha_rgrad) {
  return gaib_gat_softmax_bwd_alpha_ex(ctx, g, len, heads, d_feat, d_norm_scores, d_norm_scores_grad, d_temp_scores,
                                       epsilon, d_scores, d_alpha_lgrad, d_alpha_rgrad, nullptr, nullptr, nullptr);
}

extern "C" int gaib_gat_softmax_bwd_alpha(gaib_ctx* ctx, gaib_graph* g, int len, const float* d_feat,
                                          const float* d_norm_scores,
                                          const float* d_norm_scores_grad,
                                          const float* d_temp_scores, float epsilon,
                                          float* d_scores, float* d_alpha_lgrad,
                                          float* d_alpha_rgrad) {
  return gaib_gat_softmax_bwd_alpha_mh(ctx, g, len, 1, d_feat, d_norm_scores, d_norm_scores_grad, d_temp_scores,
                                       epsilon, d_scores, d_alpha_lgrad, d_alpha_rgrad);
}

extern "C" int gaib_edge_transpose_mh(gaib_ctx* ctx, gaib_graph* g, int heads, const float* d_in_e,
                                      float* d_out_e) {
  GAIB_CHECK(ctx && g, "gaib_edge_transpose: NULL ctx/graph");
  GAIB_CHECK(heads >= 1, "gaib_edge_transpose: heads must be >= 1");
  if (g->ne == 0) return GAIB_OK;
  GAIB_CHECK(d_in_e && d_out_e && d_in_e != d_out_e, "gaib_edge_transpose: bad pointers");
  GAIB_HIP(hipSetDevice(ctx->device));
  GAIB_TRY(gaib_graph_ensure_rev(ctx, g));
  // rev is an involution on a structurally symmetric graph: out[rev[e]] = in[e]  <=>
  // out[e] = in[rev[e]]; the gather form keeps the stores coalesced.
  edge_gather_kernel<<<(unsigned)cdiv64(g->ne * heads, 256), 256, 0, ctx->stream>>>(g->ne, heads, g->rev,
                                                                                  d_in_e, d_out_e);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_edge_transpose(gaib_ctx* ctx, gaib_graph* g, const float* d_in_e,
                                   float* d_out_e) {
  return gaib_edge_transpose_mh(ctx, g, 1, d_in_e, d_out_e);
}
