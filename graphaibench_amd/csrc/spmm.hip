// spmm.hip -- CSR SpMM neighbour aggregation for gfx950 (the hot loop).
//
//   out[i,:] = sum_{e in row i} w_e * in[col_e,:]
//
// replaces GCN_Aggregator::update_all (src/gnn/gconv/gcn_aggregator.cpp:48-77), the two
// SAGE_Aggregator loops (sage_aggregator.cpp:7-54), the file-static update_all of the GAT
// aggregator (gat_aggregator.cpp:26-45) and, on the reference's CUDA side, update_all_gcn /
// update_all_sage / reduce_warp / reduce_cta (include/gnn/graph_operations.h:8-178).
//
// Design (MI355X):
//   * HBM-bound gather: per aggregated edge one 4*len-byte feature row + 4 B colidx
//     (+ 4 B weight).  No LDS staging of feature rows: a 64-lane wave already covers a
//     512-B row with one dwordx2 load per lane, and up to U such loads are kept in flight
//     per wave (<= 64 VGPRs -> 8 waves/SIMD), which is what covers the ~2 us loaded HBM
//     latency.  colidx / weights are read coalesced, 64 edges per wave instruction, and
//     broadcast with v_readlane (SGPR) so the row base address is scalar.
//   * one wave per row ("w64" kernels) when a row needs >= 32 lanes; for narrow rows
//     (len/VEC < 32) a wave is cut into 64/G groups, one row per group ("sub" kernels).
//   * rows are summed in CSR order with separate multiply and add (no FMA), i.e. exactly
//     the OpenMP loop's rounding: results are bit-identical for rows up to the heavy
//     threshold.
//   * power-law tail: rows with more than `heavy_thr` edges are skipped by the light kernel
//     and handled by a workgroup-per-row kernel (16 waves split the edge list, partial sums
//     meet in LDS and are added in wave order -> deterministic).
//   * blockIdx -> row-block mapping is XCD-aware: consecutive row blocks land on the same
//     XCD (blocks b and b+8 share one), so neighbouring rows share that XCD's 4 MB L2.
#include <algorithm>
#include "spmm_kernels.h"

namespace {

// ---- dense graphs: aggregation by ordered 64-edge chunks -------------------------------------------------------------
// Where rows have hundreds of edges and the feature table sits in the Infinity Cache but not in the 4 MB L2 (reddit:
// 490 edges per row over 60 MB), the row-per-wave kernels gather from all over the table at any moment.  The chunk
// list of the graph (SDDMM's, ordered by column block) turns that into a sweep: a wave sums the 64 edges of one chunk
// -- G lanes x 16 B per edge, 64/G edges per instruction -- into a partial row, a second kernel adds a row's partials in
// row order.  Fixed order, so deterministic, but not the CSR-order sum of the one-row kernels (the oracle's order).
// HT > 0 (WMODE 3, heads == HT in {4, 8, 16}): the chunk's [64][HT] weight block is read once, one edge per lane
// (HT/4 16-byte loads), parked in the wave's LDS slice with a row stride of HT + 1 floats and picked up per (edge, head)
// from there: 2 + 2 wave instructions per chunk instead of one 4-byte global load per lane and edge.
// E = uint16_t: the table holds bf16 bits (a lane's 4 elements are one 8-B load, widened exactly); sums as for fp32.
// E = fp8_t: e4m3 bytes with row scales (one 4-B load, widened exactly; the scale of an edge's column rides in its weight).
template <int G, int WMODE, int HT = 0, typename E = float>
__global__ __launch_bounds__(256) void spmm_chunk_kernel(int64_t n_chunks, const uint32_t* chunk_row,
                                                         const uint32_t* chunk_ebase, const uint32_t* chunk_start,
                                                         SpmmArgs a, float* partial) {
  constexpr int U = G < 8 ? G : 8;
  constexpr bool MH = WMODE >= 3;
  constexpr int WS = HT + 1;  // LDS row stride (floats)
  __shared__ float wlds[HT > 0 ? 4 * 64 * WS : 1];
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_chunks) return;
  const int lane = threadIdx.x & 63;
  const int sl = lane & (G - 1), gbase = lane & ~(G - 1);
  const int64_t row = chunk_row[c];
  const int64_t eb = chunk_ebase[c];
  const int64_t rb = a.rowptr[row];
  const int64_t rem = a.rowptr[row + 1] - eb;
  const int n = rem < 64 ? (int)rem : 64;
  const uint32_t cl = a.col[eb + (lane < n ? lane : 0)];
  float wl = 0.f;  // weight of edge `lane` of the chunk (0 past the end)
  if (lane < n) {
    if constexpr (WMODE == 0) wl = a.rw[row];
    else if constexpr (WMODE == 1 || WMODE == 2) wl = load_edge_w<WMODE>(a, eb + lane);
    if constexpr (sizeof(E) == 1) wl = fp8_fold_scale<0>(a, cl, wl);
  }
  const bool colok = sl * 4 < a.ncols;
  const int coff = colok ? sl * 4 : 0;
  const int head = MH ? coff / a.dh : 0;
  float* wd = wlds + (HT > 0 ? (threadIdx.x >> 6) * 64 * WS : 0);
  if constexpr (HT > 0) {
    f32x4_t wv[HT / 4];
    const float* src = a.ew + (eb + (lane < n ? lane : 0)) * HT;
#pragma unroll
    for (int q = 0; q < HT / 4; ++q) wv[q] = reinterpret_cast<const f32x4_t*>(src)[q];
#pragma unroll
    for (int q = 0; q < HT / 4; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) wd[lane * WS + 4 * q + k] = lane < n ? wv[q][k] : 0.f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // LDS operations of one wave complete in order
  }
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < G; j += U) {
    f32x4_t x[U];
    float w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ei = gbase + j + u;  // edge of the chunk this group handles now
      const uint32_t cj = (uint32_t)__shfl((int)cl, ei, 64);
      if constexpr (sizeof(E) == 1)
        x[u] = load_elems<4, E>(reinterpret_cast<const char*>(a.in) + ((int64_t)cj * a.ld + coff));
      else if constexpr (sizeof(E) == 2)
        x[u] = load_elems<4, E>(reinterpret_cast<const char*>(a.in) + ((int64_t)cj * a.ld + coff) * 2);
      else
        x[u] = *reinterpret_cast<const f32x4_t*>(a.in + (int64_t)cj * a.ld + coff);
      if constexpr (HT > 0) w[u] = wd[ei * WS + head];
      else if constexpr (MH) w[u] = ei < n ? load_edge_w<WMODE>(a, eb + ei, head) : 0.f;
      else w[u] = __shfl(wl, ei, 64);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // lanes past the end of a short chunk gathered the row of the chunk's FIRST edge: select the product, do not rely
      // on a zero weight (0 * Inf = NaN would enter the partial sum; the row kernels never touch non-existent edges)
      const bool live = gbase + j + u < n;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float t = live ? w[u] * x[u][k] : 0.f;
        acc[k] = acc[k] + t;
      }
    }
  }
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
  }
  const int64_t slot = (int64_t)chunk_start[row] + (eb - rb) / 64;
  if (gbase == 0 && colok) *reinterpret_cast<f32x4_t*>(partial + slot * a.ncols + coff) = acc;
}

// out[row] (+)= sum of the row's chunk partials, in row order.  One wave per row, 16 B per lane (ncols <= 256).
__global__ __launch_bounds__(256) void spmm_chunk_reduce_kernel(SpmmArgs a, const uint32_t* chunk_start,
                                                                const float* partial) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.n_rows) return;
  const int lane = threadIdx.x & 63;
  if (lane * 4 >= a.ncols) return;
  const int64_t c0 = chunk_start[row], c1 = chunk_start[row + 1];
  float* o = a.out + row * a.ldo + lane * 4;
  f32x4_t s = {0.f, 0.f, 0.f, 0.f};
  if (a.accumulate) s = *reinterpret_cast<const f32x4_t*>(o);
  const float* p = partial + lane * 4;
  int64_t k = c0;
  for (; k + 4 <= c1; k += 4) {
    f32x4_t t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = *reinterpret_cast<const f32x4_t*>(p + (k + u) * a.ncols);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += t[u][q];
  }
  for (; k < c1; ++k) {
    const f32x4_t t = *reinterpret_cast<const f32x4_t*>(p + k * a.ncols);
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += t[q];
  }
  if (a.relu) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = s[q] > 0.f ? s[q] : 0.f;
  }
  *reinterpret_cast<f32x4_t*>(o) = s;
}

template <int WMODE, typename E = float>
int launch_chunked(gaib_ctx* ctx, gaib_graph* g, const SpmmArgs& a) {
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (size_t)g->n_chunks * a.ncols + 256));
  float* partial = (float*)ctx->ws;
  const unsigned grid = (unsigned)cdiv64(g->n_chunks > 0 ? g->n_chunks : 1, 4);
  const int lanes = (a.ncols + 3) / 4;
  {
    // col + gathered row + the edge's weights; a partial row per chunk written (and read again by the reduction)
    const double wb = WMODE == 0 ? 0.0 : (WMODE >= 3 ? 4.0 * a.heads : 4.0);
    ProfScope ps(ctx, sizeof(E) == 2 ? "spmm_bf16_chunk" : (sizeof(E) == 1 ? "spmm_fp8_chunk" : "spmm_chunk"),
                 (double)g->ne * ((double)sizeof(E) * a.ncols + 4.0 + wb) + (double)g->n_chunks * 4.0 * a.ncols,
                 2.0 * (double)g->ne * a.ncols);
#define GAIB_CHUNK(GG) \
  spmm_chunk_kernel<GG, WMODE, 0, E><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, a, partial)
#define GAIB_CHUNK_H(GG, HH) \
  spmm_chunk_kernel<GG, 3, HH><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, a, partial)
    const bool w16 = WMODE == 3 && (((uintptr_t)a.ew) & 15) == 0;
    if (w16 && lanes > 8 && lanes <= 16 && a.heads == 8) GAIB_CHUNK_H(16, 8);
    else if (w16 && lanes > 8 && lanes <= 16 && a.heads == 4) GAIB_CHUNK_H(16, 4);
    else if (w16 && lanes > 8 && lanes <= 16 && a.heads == 16) GAIB_CHUNK_H(16, 16);
    else if (w16 && lanes > 16 && lanes <= 32 && a.heads == 8) GAIB_CHUNK_H(32, 8);
    else if (w16 && lanes > 32 && a.heads == 8) GAIB_CHUNK_H(64, 8);
    else if (lanes <= 1) GAIB_CHUNK(1);
    else if (lanes <= 2) GAIB_CHUNK(2);
    else if (lanes <= 4) GAIB_CHUNK(4);
    else if (lanes <= 8) GAIB_CHUNK(8);
    else if (lanes <= 16) GAIB_CHUNK(16);
    else if (lanes <= 32) GAIB_CHUNK(32);
    else GAIB_CHUNK(64);
#undef GAIB_CHUNK
#undef GAIB_CHUNK_H
    GAIB_LAUNCH_CHECK();
  }
  ProfScope ps(ctx, "spmm_chunk_reduce", ((double)g->n_chunks + (double)a.n_rows * (a.accumulate ? 2 : 1)) * 4.0 * a.ncols);
  spmm_chunk_reduce_kernel<<<(unsigned)cdiv64(a.n_rows, 4), 256, 0, ctx->stream>>>(a, g->chunk_start, partial);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// out[r][0..lp) = in[r][0..len) followed by zeros; lp % 4 == 0, out 16-B aligned.  One float4 of `out` per thread.
__global__ __launch_bounds__(256) void pad_rows_kernel(int64_t n4, int len, int lp4, const float* in, f32x4_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / lp4;
    const int c = (int)(i - r * lp4) * 4;
    const float* src = in + r * len + c;
    f32x4_t v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = c + k < len ? src[k] : 0.f;
    out[i] = v;
  }
}

// 128-B lines a gathered row of `bytes` bytes touches on average when rows are `bytes` apart (any 4-B alignment) ...
inline double lines_packed(int bytes) { return 1.0 + (bytes - 4) / 128.0; }
// ... and when rows start on 64-B boundaries `stride` bytes apart (stride % 64 == 0)
inline double lines_strided(int bytes, int stride) {
  const int at0 = (bytes + 127) / 128, at64 = (bytes + 64 + 127) / 128;
  return stride % 128 == 0 ? at0 : 0.5 * (at0 + at64);
}

}  // namespace

// Rows whose byte length is not a multiple of 64 straddle more 128-B lines than they fill (a 188-B row of the
// 47-class output layer touches 2.44 lines on average, 2 when rows start on 64-B boundaries), and the gather time
// follows the lines touched: products, D = 47: 5.28 ms, D = 48: 4.04 ms.  Where re-striding saves more than 10 %
// of the lines, the input table is copied once into rows of whole 64-B pieces (0.9 GB of streaming traffic against
// 40 GB of gathers at products / 47) and gathered from there; output rows keep the caller's stride.
// Returns the padded row stride in floats, 0 where the fp32 table is gathered as it is.
static int64_t pad_stride_floats(const gaib_ctx* ctx, const gaib_graph* g, int len, bool part) {
  const int bytes = len * 4, stride = (bytes + 63) & ~63;
  // (not inside a side-stream section: the copy buffer belongs to the main stream's calls)
  if (ctx->spmm_pad && !part && !ctx->forked && len > 16 && stride != bytes && g->ne > 4 * g->nc &&
      lines_strided(bytes, stride) < 0.9 * lines_packed(bytes))
    return stride / 4;
  return 0;
}

// The same rule on bf16 rows (2 B per element, rows at any 2-B alignment when packed): a 47-wide row is 94 B -- 1.72 lines
// packed, one line from a 128-B stride --, a 100-wide one 200 B -- 2.55 lines packed, two from a 256-B stride.  No copy pass
// here: the cast that makes the bf16 table writes it at this stride (gaib_cast_f32_bf16_rows), the aggregation reads it
// through gaib_spmm_bf16_ld / gaib_spmm_gemm(2)_bf16_ld.  Returns the stride in elements, len where nothing is gained.
static int64_t bf16_row_stride(const gaib_ctx* ctx, const gaib_graph* g, int len) {
  const int bytes = len * 2, stride = (bytes + 63) & ~63;
  if (ctx->spmm_bf16_pad && !g->row_map && len > 16 && stride != bytes && g->ne > 4 * g->nc &&
      lines_strided(bytes, stride) < 0.9 * (1.0 + (bytes - 2) / 128.0))
    return stride / 2;
  return len;
}

extern "C" int gaib_bf16_row_stride(gaib_ctx* ctx, gaib_graph* g, int len, int64_t* ld) {
  GAIB_CHECK(ctx && g && ld, "gaib_bf16_row_stride: NULL argument");
  GAIB_CHECK(len >= 0, "gaib_bf16_row_stride: len < 0");
  *ld = bf16_row_stride(ctx, g, len);
  return GAIB_OK;
}

// size of a table of `rows` rows of `ld` elements as the buffer-descriptor path sees it: 0 where it reaches 4 GB (64-bit addresses then)
static uint32_t buf_bytes(int64_t rows, int64_t ld, bool bf16, bool fp8 = false) {
  const int64_t b = rows * ld * (fp8 ? 1 : (bf16 ? 2 : 4));
  return b < ((int64_t)1 << 32) ? (uint32_t)b : 0u;
}

// row stride (elements) the gather reads the table at: a bf16 table's own (ld_bf16 > 0: the caller cast it that way), an fp32
// table's re-strided copy where pad_stride_floats makes one
static int64_t gather_ld(const gaib_ctx* ctx, const gaib_graph* g, int len, bool part, bool bf16, int64_t ld_bf16) {
  if (bf16) return ld_bf16 > 0 ? ld_bf16 : len;  // (and an fp8 table's: callers pass bf16 || fp8)
  const int64_t lp = pad_stride_floats(ctx, g, len, part);
  return lp > 0 ? lp : len;
}

// fills the launch arguments shared by every aggregation path; *wmode = kernel weight mode
// d_in2 / n_first: column ids >= n_first index the second table d_in2 (row id - n_first) -- NULL: one table
// bf16: d_in (and d_in2) hold bf16 bits (gaib_spmm_bf16, gaib_spmm_part_bf16): gathered as they are (no re-strided copy, no
// cold-column flags), and the buffer-descriptor path is chosen by the tables' bf16 byte sizes
// ld_bf16 > 0: the row stride of a bf16 table in elements (gaib_spmm_bf16_ld; the caller cast it that way: gaib_cast_f32_bf16_rows)
// -- it enters the gather addresses, the descriptor size and the 4 GB test, nothing else
// fp8: d_in holds e4m3 bytes at the row stride ld_bf16 (bytes; gaib_spmm_fp8): gathered as they are like a bf16 table, but WITH the
// cold-column flags of gather mode 3 (the row kernels' scale fetch masks them); the caller points a.in2 at the row scales
static int spmm_setup(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len,
                      const float* d_in, float* d_out, int flags, int heads, SpmmArgs* pa, int* wmode,
                      const float* d_in2 = nullptr, int64_t n_first = 0, bool bf16 = false, int64_t ld_bf16 = 0, bool fp8 = false) {
  SpmmArgs& a = *pa;
  const bool part = g->row_map != nullptr || d_in2 != nullptr;  // a row class of a partition (spmm_part.hip)
  GAIB_CHECK(!d_in2 || (n_first >= 0 && n_first <= g->nc), "gaib_spmm: n_first (%lld) outside the %lld columns",
             (long long)n_first, (long long)g->nc);
  GAIB_HIP(hipSetDevice(ctx->device));
  GAIB_TRY(gaib_graph_ensure_heavy(ctx, g, ctx->spmm_heavy_threshold));
  a.rowptr = g->rowptr;
  a.col = g->colidx;
  a.rw = nullptr;
  a.ew = nullptr;
  a.rev = nullptr;
  a.in = d_in;
  a.out = d_out;
  a.ld = len;
  a.ncols = len;
  a.n_rows = (int)g->nv;
  a.heavy_thr = g->heavy_thr;
  a.row_list = nullptr;
  a.row_order = nullptr;
  a.nblocks = 0;
  a.per_xcd = 0;
  a.xcd_chunk = 0;
  a.accumulate = (flags & GAIB_ACCUMULATE) ? 1 : 0;
  a.relu = (flags & GAIB_RELU) ? 1 : 0;
  a.heads = heads;
  a.dh = heads > 0 ? len / heads : len;
  a.col_flagged = nullptr;
  a.compact = 0;
  a.row_map = g->row_map;
  a.in2 = d_in2;
  a.n_first = d_in2 ? (uint32_t)n_first : 0xffffffffu;
  a.in2_bytes = 0;
  a.col0 = 0;
  // gather mode 3 (the row kernels of gaib_spmm): the graph's flagged column ids.  Never built inside a capture: a recorded call
  // whose flags do not exist yet gathers with the default policy.
  if (!part && !bf16 && ctx->spmm_gather_mode == 3 && g->nc == g->nv && !g->col_vdata) {
    const int64_t want = gaib_hot_rows_wanted(ctx, g);
    if (!ctx->capturing) GAIB_TRY(gaib_graph_ensure_hot_flags(ctx, g, want));
    if (g->colidx_flagged && g->hot_rows == want) a.col_flagged = g->colidx_flagged;
  }
  a.ldo = len;
  // odd-width tables: gathered from a copy re-strided to whole 64-B pieces where that saves lines (pad_stride_floats)
  {
    const int64_t lp_pad = bf16 || fp8 ? 0 : pad_stride_floats(ctx, g, len, part);
    if (lp_pad > 0) {
      const int lp = (int)lp_pad;
      GAIB_TRY(gaib_pad_reserve(ctx, (size_t)g->nc * (size_t)lp * 4));
      const int64_t n4 = g->nc * (int64_t)(lp / 4);
      const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(n4, 256), (int64_t)ctx->num_cus * 16);
      pad_rows_kernel<<<grid, 256, 0, ctx->stream>>>(n4, len, lp / 4, d_in, reinterpret_cast<f32x4_t*>(ctx->pad));
      GAIB_LAUNCH_CHECK();
      a.in = reinterpret_cast<const float*>(ctx->pad);
      a.ld = lp;
    }
  }
  if ((bf16 || fp8) && ld_bf16 > 0) a.ld = ld_bf16;
  // feature table = nc rows of a.ld elements (4 B, 2 B in bf16, 1 B in fp8); the 32-bit buffer path needs it below 4 GB
  a.in_bytes = buf_bytes(d_in2 ? n_first : g->nc, a.ld, bf16, fp8);
  if (d_in2) a.in2_bytes = buf_bytes(g->nc - n_first, a.ld, bf16);
  switch (weight_kind) {
    case GAIB_W_GCN:
      GAIB_TRY(gaib_graph_ensure_w_gcn(ctx, g));
      a.ew = g->w_gcn;
      *wmode = 1;
      return GAIB_OK;
    case GAIB_W_MEAN:
      GAIB_TRY(gaib_graph_ensure_inv_deg(ctx, g));
      a.rw = g->inv_deg;
      *wmode = 0;
      return GAIB_OK;
    case GAIB_W_MEAN_T:
      GAIB_TRY(gaib_graph_ensure_w_mean_t(ctx, g));
      a.ew = g->w_mean_t;
      *wmode = 1;
      return GAIB_OK;
    case GAIB_W_EDGE:
      GAIB_CHECK(d_edge_w || g->ne == 0, "gaib_spmm: GAIB_W_EDGE needs d_edge_w");
      a.ew = d_edge_w;
      *wmode = heads > 1 ? 3 : 1;
      return GAIB_OK;
    case GAIB_W_EDGE_T:
      GAIB_CHECK(d_edge_w || g->ne == 0, "gaib_spmm: GAIB_W_EDGE_T needs d_edge_w");
      GAIB_TRY(gaib_graph_ensure_rev(ctx, g));
      a.ew = d_edge_w;
      a.rev = g->rev;
      *wmode = heads > 1 ? 4 : 2;
      return GAIB_OK;
    default:
      gaib_set_error("gaib_spmm: unknown weight_kind %d", weight_kind);
      return GAIB_ERR_INVALID;
  }
}

// Where the ordered-chunk aggregation pays (scripts/ab_chunked.py, microbench_layers.py): a chunk of 64 edges of a row
// with d edges spans 64/d of the columns, so it is L2-sized only on long rows -- on the reddit shape the rows above the
// heavy threshold hold half of the edges and the two aggregations of a layer drop from 6.65 to 4.1 ms, on uniform random
// graphs of the same density nothing is gained (-12 % at 256 edges per row, +5-8 % at 32-128).  Rule: a table that can
// live in the Infinity Cache and at least a quarter of the edges in heavy rows.
static bool chunk_rule(gaib_ctx* ctx, gaib_graph* g, int64_t ld) {
  if (gaib_graph_ensure_heavy(ctx, g, ctx->spmm_heavy_threshold) != GAIB_OK) return false;
  return g->nc * ld * 4 <= ((int64_t)512 << 20) && 4 * g->heavy_edges >= g->ne && g->ne > 0;
}

static int spmm_impl(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len,
                     const float* d_in, float* d_out, int flags, int heads = 1, const float* d_in2 = nullptr,
                     int64_t n_first = 0) {
  GAIB_CHECK(ctx && g, "gaib_spmm: NULL ctx/graph");
  GAIB_CHECK(len >= 0, "gaib_spmm: len < 0");
  GAIB_CHECK(ctx->device == g->device, "gaib_spmm: graph lives on device %d, ctx on %d", g->device,
             ctx->device);
  if (len == 0 || g->nv == 0) return GAIB_OK;
  GAIB_CHECK(d_in && d_out, "gaib_spmm: NULL feature pointer");
  GAIB_CHECK(d_in != d_out, "gaib_spmm: in and out must not alias");
  SpmmArgs a;
  int wmode = 0;
  GAIB_TRY(spmm_setup(ctx, g, weight_kind, d_edge_w, len, d_in, d_out, flags, heads, &a, &wmode, d_in2, n_first));
  if (g->row_map || d_in2) {
    GAIB_CHECK(d_in2 != d_out, "gaib_spmm: in2 and out must not alias");
    GAIB_CHECK(heads == 1 && wmode <= 1, "gaib_spmm: a row class of a partition aggregates with GAIB_W_GCN / _MEAN / _MEAN_T / "
                                          "single-head _EDGE weights (got kind %d, %d heads)", weight_kind, heads);
    return gaib_spmm_part_plain(ctx, g, a, wmode, len);
  }
  // dense graphs over a table that fits the Infinity Cache: ordered chunks (see spmm_chunk_kernel)
  const bool chunk_shape = len % 4 == 0 && len <= 256 && a.ld % 4 == 0 && a.ldo % 4 == 0 && g->ne > 0 &&
                           ((((uintptr_t)a.in | (uintptr_t)a.out) & 15) == 0) && (wmode < 3 || a.dh % 4 == 0);
  const bool chunk_auto = ctx->spmm_chunked < 0 && chunk_rule(ctx, g, a.ld);
  if (chunk_shape && (ctx->spmm_chunked == 1 || (ctx->spmm_chunked < 0 && chunk_auto))) {
    switch (wmode) {
      case 0: return launch_chunked<0>(ctx, g, a);
      case 1: return launch_chunked<1>(ctx, g, a);
      case 2: return launch_chunked<2>(ctx, g, a);
      case 3: return launch_chunked<3>(ctx, g, a);
      default: return launch_chunked<4>(ctx, g, a);
    }
  }
  switch (wmode) {
    case 0: return dispatch_vec<0>(ctx, g, a, len);
    case 1: return dispatch_vec<1>(ctx, g, a, len);
    case 2: return dispatch_vec<2>(ctx, g, a, len);
    case 3: return dispatch_vec<3>(ctx, g, a, len);
    default: return dispatch_vec<4>(ctx, g, a, len);
  }
}

extern "C" int gaib_spmm(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w,
                         int len, const float* d_in, float* d_out) {
  return spmm_impl(ctx, g, weight_kind, d_edge_w, len, d_in, d_out, 0);
}

extern "C" int gaib_spmm_acc(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w,
                             int len, const float* d_in, float* d_out) {
  return spmm_impl(ctx, g, weight_kind, d_edge_w, len, d_in, d_out, GAIB_ACCUMULATE);
}

extern "C" int gaib_spmm_ex(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w,
                            int len, const float* d_in, float* d_out, int flags) {
  return spmm_impl(ctx, g, weight_kind, d_edge_w, len, d_in, d_out, flags);
}

extern "C" int gaib_spmm_2t(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len,
                            const float* d_in, const float* d_in2, int64_t n_first, float* d_out, int flags) {
  GAIB_CHECK(ctx && g, "gaib_spmm_2t: NULL ctx/graph");
  GAIB_CHECK(d_in2 || n_first >= g->nc || g->nv == 0 || g->ne == 0, "gaib_spmm_2t: NULL second table with columns beyond n_first");
  return spmm_impl(ctx, g, weight_kind, d_edge_w, len, d_in, d_out, flags, 1, d_in2, n_first);
}

// ---- the fused aggregation: agg = A.in ; out = act(agg . op(W) [+ rows2 . op(W2)]) ----------------------------------------------
// Fused on the matrix cores when the shape allows, otherwise gaib_spmm followed by gaib_sgemm (same results up to summation
// order).  Every gaib_spmm_gemm* entry fills ONE description of its call (GemmCall), ONE function decides the route and the form
// of the fused launch (gemm_route), and each route has ONE executor (spmm_gemm_run).
struct GemmCall {
  int weight_kind;
  const float* d_edge_w;
  int len_in;
  const float* d_in;  // the table: fp32, or bf16 bits (bf16)
  float* d_agg;
  const float* d_W;
  int transW;
  const float *d_rows2, *d_W2;  // the second product: both or neither
  int len_out;
  float* d_out;
  int flags;
  // set by name by the entries that have them
  const float* d_in2 = nullptr;  // second table, indexed by column ids >= n_first (row id - n_first): gaib_spmm_gemm_2t / _part_bf16
  int64_t n_first = 0, ld = 0;   // ld: a bf16 table's rows are this many elements apart (0: len_in)
  bool bf16 = false;             // d_in (and d_in2) hold bf16 bits
  const void* d_zs = nullptr;  // the zero-suppressed image of d_in (gaib_pack_zs, or gaib_pack_zs_wide at 256 columns)
  bool fp8 = false;                // d_in holds e4m3 bytes at the row stride ld (bytes), d_scale the row scales (gaib_spmm_gemm_fp8)
  const float* d_scale = nullptr;
};

// the routes (the table stands at gemm_route): nothing to do | one fused launch | the neighbour product fused, then the accumulating
// product | one fused launch per 128-column K-slab | aggregate, then multiply | GAIB_ERR_UNSUPPORTED with its message
enum GemmRouteKind { ROUTE_NONE, ROUTE_FUSED, ROUTE_FUSED_THEN_GEMM, ROUTE_KSLABS, ROUTE_UNFUSED, ROUTE_REFUSED };
struct GemmRoute {
  GemmRouteKind kind;
  FuseForm form;  // of the fused launch (ROUTE_KSLABS: of the first slab's)
};

// the weight kinds the fused kernels take
static bool fuse_kind_ok(int k) { return k == GAIB_W_GCN || k == GAIB_W_MEAN || k == GAIB_W_MEAN_T || k == GAIB_W_EDGE; }

// short rows (fewer than 12 edges per row on average: halo-column halves, citation graphs) take the edge-stream form
// (scripts/ab_flat.py: -34 % at 3 edges per row, -20 % at 5, even at 12, +2 % at 30); option spmm_flat forces or forbids it
static bool edge_stream_rule(const gaib_ctx* ctx, const gaib_graph* g) {
  return ctx->spmm_flat >= 1 || (ctx->spmm_flat < 0 && g->ne < 12 * g->nv);
}

// The shape-only part of "can the product ride on the aggregation in one launch": the strip height of that launch, 0 where there
// is none.  The weight matrices [len_out x (len_in+4)] and 16 row strips must fit the CU's 160 KB of LDS; 65..128 columns need
// 8-byte lanes.  (What the row classes of a partition must agree on: they share one output matrix, so either every class runs
// the fused kernel or none does -- host/aggregators.cpp asks gaib_spmm_gemm_fusable first.)
static int fuse_shape_strip(const gaib_ctx* ctx, int weight_kind, int len_in, int len_out, bool dual) {
  if (!ctx->spmm_fuse || len_in < 1 || len_in > 128 || len_out < 1) return 0;
  if ((len_in > 64 && len_in % 2 != 0) || !fuse_kind_ok(weight_kind)) return 0;
  return fuse_strip_rows(len_in <= 64 ? 64 : 128, len_out, dual);
}

extern "C" int gaib_spmm_gemm_fusable(gaib_ctx* ctx, int weight_kind, int len_in, int len_out, int dual) {
  return ctx && fuse_shape_strip(ctx, weight_kind, len_in, len_out, dual != 0) != 0 ? 1 : 0;
}

// option spmm_tile_xcd -> FuseForm::tile_xcd (0 = global counter, else log2(chunk length in tiles) + 1).
// -1 (default): by the graph's numbering -- XCD-affine chunks of 1024 tiles when at least a quarter of the edges stay
// within 32 768 ids of their row, else the global counter (scripts/ab_tile_xcd.py, products size, D = 128: a numbering with
// planted locality 5.94 -> 5.01 ms at 512-1024 tiles per chunk, a random one 7.60 -> 7.80 ms with ANY chunk length: hence the
// rule instead of one setting).  1 = the round-2 form (16-tile chunks); n = chunk length, rounded down to 2^k.
static int tile_xcd_arg(gaib_ctx* ctx, gaib_graph* g) {
  int v = ctx->spmm_tile_xcd;
  if (v < 0) {
    if (gaib_graph_ensure_locality(ctx, g) != GAIB_OK) return 0;
    v = g->near_frac >= 0.25f ? 1024 : 0;
  }
  if (v <= 0) return 0;
  if (v == 1) v = 16;
  int sh = 0;
  while ((2 << sh) <= v) ++sh;
  return sh + 1;
}

// Option spmm_hot_cold for a launch whose form has the hot/cold gather (fuse_form: 8-B lanes, row form, 8-row strip, one product,
// global tile counter, buffer addressing, whole graph, fp32 or zero-suppressed table): the graph's flagged column ids when the option
// resolves to on for this table, else NULL (the launch then reads the plain ids, default policy).
//   1  on wherever the form runs on a square graph without column normalisers (a column's degree is its row's)
//  -1  auto: GAIB_HOT_COLD_AUTO (common.h: what the measurement decided), a DENSE table (the packed gather measured slower
//      with the option at every hot-set size), larger than twice the 256 MiB Infinity Cache -- a table that fits is resident
//      whatever the policy -- and a numbering that is not local (near_frac < 0.25)
//   0  off
// The flags are per-graph preprocessing, built next to the heavy-row list on the first call outside a capture; inside a
// capture nothing is built: without current flags the call runs with the default policy.
static const uint32_t* hot_cold_cols(gaib_ctx* ctx, gaib_graph* g, int64_t table_bytes, bool packed) {
  if (ctx->spmm_hot_cold == 0 || ctx->spmm_gather_mode == 3) return nullptr;  // (gather mode 3 sizes the one flagged array for the L2)
  if (g->row_map || g->nc != g->nv || g->col_vdata || g->ne == 0) return nullptr;
  if (ctx->spmm_hot_cold < 0) {
    if (!GAIB_HOT_COLD_AUTO || packed || table_bytes <= ((int64_t)512 << 20)) return nullptr;
    if (g->near_frac < 0.f && (ctx->capturing || gaib_graph_ensure_locality(ctx, g) != GAIB_OK)) return nullptr;
    if (g->near_frac >= 0.25f) return nullptr;
  }
  const int64_t want = gaib_hot_rows_wanted(ctx, g);
  if (!ctx->capturing && gaib_graph_ensure_hot_flags(ctx, g, want) != GAIB_OK) return nullptr;
  return (g->colidx_flagged && g->hot_rows == want) ? g->colidx_flagged : nullptr;
}

// The form of the fused launch of a call: `dual` products on the `strip`-row strip (see the table at gemm_route).  Measures the
// numbering's locality where spmm_tile_xcd is on auto (once per graph, not inside a capture); builds nothing else.
static FuseForm fuse_form(gaib_ctx* ctx, gaib_graph* g, const GemmCall& c, bool part, bool dual, int strip, bool kslabs) {
  FuseForm fm;
  fm.vec = c.len_in <= 64 ? 1 : 2;
  fm.strip = strip;
  fm.dual = dual;
  fm.yacc = false;
  // the table(s) as the gather addresses them -- a bf16 table counts its own bytes here, the one place its real size decides
  const int64_t ld = gather_ld(ctx, g, c.len_in, part, c.bf16 || c.fp8, c.ld);
  fm.buf = ctx->spmm_addr_mode != 2 && buf_bytes(c.d_in2 ? c.n_first : g->nc, ld, c.bf16, c.fp8) != 0 &&
           (!c.d_in2 || buf_bytes(g->nc - c.n_first, ld, c.bf16) != 0);
  fm.short_rows = edge_stream_rule(ctx, g);
  fm.flat = fm.short_rows && !dual && strip == 8;
  fm.ring = fm.flat && ctx->spmm_flat_ring != 0;
  const int tile_xcd = tile_xcd_arg(ctx, g);  // (asked whatever the table kind: the locality is measured on a graph's first fused call)
  fm.tile_xcd = part || c.bf16 || c.fp8 ? 0 : tile_xcd;
  // (hot_cold: the launch has the form; run_fused asks hot_cold_cols whether the option is on and the flags exist)
  fm.hot_cold = !kslabs && !part && !c.bf16 && !c.fp8 && fm.vec == 2 && fm.buf && !dual && strip == 8 && !fm.flat && fm.tile_xcd == 0;
  return fm;
}

// The route of a call and the form of its fused launch.  Launches no aggregation and reads nothing through the table, image or
// matrix pointers (gaib_spmm_gemm_zs_route returns what it says, BEFORE the caller packs); the per-graph preprocessing it may run
// is the heavy-row list (the chunk rule reads it) and the locality of the numbering, neither inside a capture.
//
//   call and shape (fp32 view of the table), first match                                                  route
//   nv == 0 or len_out == 0                                                                               NONE
//   whole graph, spmm_chunked 1 or chunk rule; len_in % 4 == 0, in / agg 16-B aligned                     UNFUSED (ordered chunks)
//   spmm_fuse 0, a weight kind the fused kernels lack, ne == 0 on a whole graph                           UNFUSED
//   len_in <= 64, or <= 128 even with in / agg 8-B aligned; W (and W2, len_out <= 128) fit 160 KB of LDS   FUSED: 4-B / 8-B lanes; 8-row strip where it
//                                                                                                           fits next to W, else 2; two products: 2
//   the same, whole graph, two products of which W alone fits (100 -> 256)                                FUSED_THEN_GEMM: the one-product form
//   129 <= len_in <= 256 even, 8-B aligned, whole graph, ne > 0, a 128-column slab of W fits              KSLABS: per slab the one-product form, later
//                                                                                                           slabs y += ; a second product follows
//   everything else (odd above 64, > 256, unaligned)                                                      UNFUSED
//   ... and where a row class of a partition would go UNFUSED: REFUSED (the classes' rows share one output)
// "fp32 view": a bf16 table stands for its widened fp32 table -- at twice the address, the chunk rule counting fp32 bytes -- so
// both take the same route, and each route runs the bf16 gather; an fp8 table (c.fp8) likewise, at four times the address.  The
// form next to the route (fuse_form):
//   edge stream  short rows (edge_stream_rule) on the one-product 8-row strip, never on a later K-slab; a ring with spmm_flat_ring
//   addressing   buffer descriptors while every table is below 4 GB and spmm_addr_mode != 2, else 64-bit
//   tile supply  spmm_tile_xcd (XCD-affine chunks; auto: a numbering with locality); global counter on classes, bf16 and fp8 tables
//   hot/cold     spmm_hot_cold (hot_cold_cols) on 8-B lanes, 8-row strip, one product, row form, buffer addressing, global
//                counter, an fp32 or zero-suppressed table of a whole graph
// A zero-suppressed image (d_zs) has a packed gather only on FUSED at 128 columns (two products, or the 8-row strip) and on KSLABS
// at 256 columns, with buffer addressing, no edge stream on short rows, the global tile counter: any other form is REFUSED.
static int gemm_route(gaib_ctx* ctx, gaib_graph* g, const GemmCall& c, GemmRoute* r) {
  *r = GemmRoute{};
  r->kind = ROUTE_NONE;
  GAIB_CHECK(ctx && g, "gaib_spmm_gemm: NULL ctx/graph");
  GAIB_CHECK(c.len_in >= 0 && c.len_out >= 0, "gaib_spmm_gemm: negative length");
  GAIB_CHECK(ctx->device == g->device, "gaib_spmm_gemm: graph lives on device %d, ctx on %d", g->device, ctx->device);
  GAIB_CHECK((c.flags & ~(GAIB_RELU | GAIB_AGG_SCRATCH | GAIB_ACCUMULATE | GAIB_OVERLAPS_TRANSFER)) == 0,
             "gaib_spmm_gemm: unsupported flags %d", c.flags);
  GAIB_CHECK((c.d_rows2 == nullptr) == (c.d_W2 == nullptr), "gaib_spmm_gemm2: rows2 and W2 go together");
  if (g->nv == 0 || c.len_out == 0) return GAIB_OK;
  GAIB_CHECK(c.d_in && c.d_agg && c.d_W && c.d_out, "gaib_spmm_gemm: NULL pointer");
  GAIB_CHECK(c.d_in != c.d_agg && c.d_agg != c.d_out && c.d_in != c.d_out && c.d_rows2 != c.d_out && c.d_rows2 != c.d_agg,
             "gaib_spmm_gemm: buffers must not alias");
  const int len_in = c.len_in, len_out = c.len_out;
  const bool dual = c.d_rows2 != nullptr;
  const bool part = g->row_map != nullptr || c.d_in2 != nullptr;  // a row class of a partition
  const uintptr_t tables = (uintptr_t)c.d_in | (uintptr_t)c.d_in2;
  const uintptr_t al = (c.fp8 ? tables << 2 : (c.bf16 ? tables << 1 : tables)) | (uintptr_t)c.d_agg;  // the fp32 view's alignment
  // dense graphs over a cache-sized table aggregate faster by ordered chunks (spmm_chunk_kernel) than row by row
  // inside the fused kernel: two kernels there
  const bool dense = !part && ctx->spmm_chunked != 0 && len_in % 4 == 0 && (al & 15) == 0 &&
                     (ctx->spmm_chunked == 1 || chunk_rule(ctx, g, len_in));
  // (a row class may be without edges -- isolated interior vertices -- and still owes its rows of y)
  const bool rows_ok = !dense && (len_in <= 64 || (al & 7) == 0) && (g->ne > 0 || part);
  const int one = rows_ok ? fuse_shape_strip(ctx, c.weight_kind, len_in, len_out, dual) : 0;
  const int one1 = rows_ok && dual && !part ? fuse_shape_strip(ctx, c.weight_kind, len_in, len_out, false) : 0;
  const int slab = !part && ctx->spmm_fuse != 0 && !dense && len_in > 128 && len_in <= 256 && len_in % 2 == 0 && (al & 7) == 0 &&
                           len_out >= 1 && g->ne > 0 && fuse_kind_ok(c.weight_kind)
                       ? fuse_strip_rows(128, len_out, false)
                       : 0;
  if (one == 0 && one1 != 0) r->kind = ROUTE_FUSED_THEN_GEMM, r->form = fuse_form(ctx, g, c, part, false, one1, false);
  else if (slab != 0) r->kind = ROUTE_KSLABS, r->form = fuse_form(ctx, g, c, part, false, slab, true);
  else if (one != 0) r->kind = ROUTE_FUSED, r->form = fuse_form(ctx, g, c, part, dual, one, false);
  else r->kind = ROUTE_UNFUSED;
  const FuseForm& fm = r->form;
  if (c.d_zs) {
    // 256 columns (a wide image): the K-slab route's launches are one-product launches whatever `dual` says.  129 .. 255: a second
    // slab narrower than 128 columns has no packed form.  Nor have the 2-row strip with one product, the edge stream the dense call
    // takes on short rows (20-34 % faster than the row form at 3-5 edges per row), the XCD-affine supply, 64-bit addressing.
    const bool wide = len_in == 256;
    const bool packed = (wide ? r->kind == ROUTE_KSLABS : (r->kind == ROUTE_FUSED && !part && len_in == 128 && (fm.dual || fm.strip == 8))) &&
                        fm.buf && !(fm.short_rows && (wide || !fm.dual)) && fm.tile_xcd == 0 && ((uintptr_t)c.d_zs & 127) == 0;
    if (!packed) {
      r->kind = ROUTE_REFUSED;
      gaib_set_error("gaib_spmm_gemm_zs: no zero-suppressed gather for this call (whole graph, 128 columns on the one-launch fused route "
                     "or 256 columns -- a wide image -- on the K-slab route, in the row form -- 8-row strip, two products or a K-slab, "
                     "no edge stream, global tile counter --, table below 4 GB, buffer addressing, image on a 128-B boundary)");
      return GAIB_ERR_UNSUPPORTED;
    }
  }
  if (part && r->kind == ROUTE_UNFUSED) {
    // the classes of a partition write disjoint rows of ONE output: the caller (host/aggregators.cpp) asks gaib_spmm_gemm_fusable
    // first and runs aggregation + one dense product over all rows where the answer is no.  (Nor can a class take the route of two
    // products that do not fit together: the accumulating product runs over rows [0, nv) of rows2 / out.)
    r->kind = ROUTE_REFUSED;
    gaib_set_error("gaib_spmm_gemm: a row class of a partition needs a fusable shape (len_in %d, len_out %d%s): aggregate "
                   "with gaib_spmm_ex / gaib_spmm_2t and multiply all rows at once", len_in, len_out, dual ? ", two products" : "");
    return GAIB_ERR_UNSUPPORTED;
  }
  return GAIB_OK;
}

// the executors' workspace -- op(W) (and op(W2)) k-contiguous, the heavy rows' aggregates, the tile counters -- and the FuseArgs of a launch
static int fuse_args(gaib_ctx* ctx, const gaib_graph* g, const GemmCall& c, bool dual, FuseArgs* pf) {
  const size_t wt_bytes = (sizeof(float) * (size_t)c.len_out * c.len_in + 255) & ~(size_t)255;
  const size_t hv_bytes = (sizeof(float) * (size_t)g->n_heavy * c.len_in + 255) & ~(size_t)255;
  const int nw = dual ? 2 : 1;
  GAIB_TRY(gaib_ws_reserve(ctx, nw * wt_bytes + hv_bytes + 256));
  float* hv = (float*)((char*)ctx->ws + nw * wt_bytes);
  const float* w[2] = {c.d_W, dual ? c.d_W2 : nullptr};  // with transW, [len_out x len_in]: already k-contiguous
  for (int i = 0; i < nw && !c.transW; ++i) {
    float* wt = (float*)((char*)ctx->ws + i * wt_bytes);
    transpose_small_kernel<<<(c.len_in * c.len_out + 255) / 256, 256, 0, ctx->stream>>>(c.len_in, c.len_out, w[i], wt);
    GAIB_LAUNCH_CHECK();
    w[i] = wt;
  }
  FuseArgs& f = *pf;
  f.wt = w[0];
  f.wt2 = w[1];
  f.rows2 = dual ? c.d_rows2 : nullptr;
  f.ldw = c.len_in;
  f.y = c.d_out;
  f.ldy = c.len_out;
  f.n_out = c.len_out;
  f.relu = (c.flags & GAIB_RELU) ? 1 : 0;
  f.heavy_agg = hv;
  f.heavy_rows = g->heavy_rows;
  f.n_heavy = (int)g->n_heavy;
  f.tile_counter = (int*)((char*)hv + hv_bytes);
  f.agg_in = (c.flags & GAIB_ACCUMULATE) ? c.d_agg : nullptr;
  f.overlaps_transfer = (c.flags & GAIB_OVERLAPS_TRANSFER) ? 1 : 0;
  f.y_accum = f.tile_xcd = 0;  // (the form's: set where the launch happens)
  return GAIB_OK;
}

// the aggregation arguments of a fused call: no agg store where the caller does not read it, partial sums through FuseArgs::agg_in
static int fuse_spmm_args(gaib_ctx* ctx, gaib_graph* g, const GemmCall& c, SpmmArgs* a, int* wmode) {
  GAIB_TRY(spmm_setup(ctx, g, c.weight_kind, c.d_edge_w, c.len_in, c.d_in, c.d_agg, 0, 1, a, wmode, c.d_in2, c.n_first, c.bf16, c.ld, c.fp8));
  if (c.fp8) a->in2 = c.d_scale;
  a->accumulate = 0;
  a->col_flagged = nullptr;
  if (c.flags & GAIB_AGG_SCRATCH) a->out = nullptr;
  return GAIB_OK;
}

// one fused launch in the form fm with the kernels of the call's table kind; k0: the first column of a K-slab (else 0)
static int launch_form(gaib_ctx* ctx, gaib_graph* g, const GemmCall& c, const FuseForm& fm, SpmmArgs a, const FuseArgs& f, int wmode, int k0) {
  float* hv = const_cast<float*>(f.heavy_agg);
  if (c.d_zs) {  // gather from the packed rows of the slab's image; the dense table stays behind them for over-capacity (half) rows
    a.in2 = a.in;
    a.in2_bytes = a.in_bytes;
    a.in = reinterpret_cast<const float*>(static_cast<const char*>(c.d_zs) + (int64_t)(k0 / 128) * g->nc * GAIB_ZS_ROW_BYTES);
    a.ld = GAIB_ZS_ROW_BYTES / 4;
    a.in_bytes = (uint32_t)(g->nc * (int64_t)GAIB_ZS_ROW_BYTES);
    return c.len_in > 128 ? gaib_spmm_kslab_zs(ctx, g, fm, a, f, hv, wmode) : gaib_spmm_fused_zs(ctx, g, fm, a, f, hv, wmode);
  }
  if (g->row_map || c.d_in2)
    return c.bf16 ? gaib_spmm_part_fused_bf16(ctx, g, fm, a, f, hv, wmode) : gaib_spmm_part_fused(ctx, g, fm, a, f, hv, wmode);
  if (c.bf16) return gaib_spmm_fused_bf16(ctx, g, fm, a, f, hv, wmode);
  if (c.fp8) return gaib_spmm_fused_fp8(ctx, g, fm, a, f, hv, wmode);
  if (fm.vec == 1) return wmode == 0 ? launch_fused<1, 0>(ctx, g, fm, a, f, hv) : launch_fused<1, 1>(ctx, g, fm, a, f, hv);
  return wmode == 0 ? launch_fused<2, 0>(ctx, g, fm, a, f, hv) : launch_fused<2, 1>(ctx, g, fm, a, f, hv);
}

static int run_fused(gaib_ctx* ctx, gaib_graph* g, const GemmCall& c, FuseForm fm) {
  SpmmArgs a;
  int wmode = 0;
  GAIB_TRY(fuse_spmm_args(ctx, g, c, &a, &wmode));
  if (fm.hot_cold) {
    a.col_flagged = hot_cold_cols(ctx, g, c.d_zs ? g->nc * (int64_t)GAIB_ZS_ROW_BYTES : g->nc * a.ld * 4, c.d_zs != nullptr);
    fm.hot_cold = a.col_flagged != nullptr;
  }
  FuseArgs f;
  GAIB_TRY(fuse_args(ctx, g, c, fm.dual, &f));
  return launch_form(ctx, g, c, fm, a, f, wmode, 0);
}

// a product that no launch carries: out (+)= rows . op(W), with the activation
static int trailing_gemm(gaib_ctx* ctx, const gaib_graph* g, const GemmCall& c, const float* rows, const float* W, int flags) {
  return gaib_sgemm_ex(ctx, 0, c.transW, g->nv, c.len_out, c.len_in, rows, W, flags | ((c.flags & GAIB_RELU) ? GAIB_RELU : 0), c.d_out);
}

// 129..256 columns (the hidden width 256 of scripts/run-sage-products.sh): op(W) does not fit LDS next to the strips, so the
// aggregation runs as two 128-column K-slabs through the same kernel, each with its [len_out x 128] slab of op(W) in LDS.  The
// gathered bytes are those of one 1-KB row gather per edge; colidx / weights are streamed twice and y is read-modify-written once
// -- against a separate pass over agg and a 2 x 2.45 M x 256 x 256 GEMM.  What a slab overrides: its column offsets, y += and the
// row form behind slab 0, the activation on the last slab only.
static int run_kslabs(gaib_ctx* ctx, gaib_graph* g, const GemmCall& c, const FuseForm& fm) {
  const bool dual = c.d_rows2 != nullptr;
  SpmmArgs a0;
  int wmode = 0;
  GAIB_TRY(fuse_spmm_args(ctx, g, c, &a0, &wmode));
  FuseArgs f0;
  GAIB_TRY(fuse_args(ctx, g, c, false, &f0));
  for (int k0 = 0; k0 < c.len_in; k0 += 128) {
    SpmmArgs a = a0;
    // (bf16: the slab offset and in_bytes count bf16 elements; the offset is one of columns, whatever the row stride)
    a.in = c.fp8    ? reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(a0.in) + k0)
           : c.bf16 ? reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(a0.in) + k0)
                    : a0.in + k0;
    a.ncols = c.len_in - k0 < 128 ? c.len_in - k0 : 128;
    if (a.out) a.out += k0;
    if (a.in_bytes) a.in_bytes -= (uint32_t)(k0 * (c.fp8 ? 1 : (c.bf16 ? 2 : 4)));
    FuseArgs f = f0;
    f.wt += k0;
    if (f.agg_in) f.agg_in += k0;
    f.heavy_agg += k0;
    f.relu = f0.relu && !dual && k0 + 128 >= c.len_in;
    FuseForm s = fm;
    s.yacc = k0 > 0;
    if (s.yacc) s.flat = s.ring = false;
    GAIB_TRY(launch_form(ctx, g, c, s, a, f, wmode, k0));
  }
  return dual ? trailing_gemm(ctx, g, c, c.d_rows2, c.d_W2, GAIB_ACCUMULATE) : GAIB_OK;
}

static int run_unfused(gaib_ctx* ctx, gaib_graph* g, const GemmCall& c) {
  const bool dual = c.d_rows2 != nullptr;
  if (c.fp8) GAIB_TRY(gaib_spmm_fp8(ctx, g, c.weight_kind, c.d_edge_w, c.len_in, c.ld, reinterpret_cast<const uint8_t*>(c.d_in),
                                    c.d_scale, c.d_agg, c.flags & GAIB_ACCUMULATE));
  else if (c.bf16) GAIB_TRY(gaib_spmm_bf16_ld(ctx, g, c.weight_kind, c.d_edge_w, c.len_in, c.ld > 0 ? c.ld : c.len_in,
                                         reinterpret_cast<const uint16_t*>(c.d_in), c.d_agg, c.flags & GAIB_ACCUMULATE));
  else GAIB_TRY(spmm_impl(ctx, g, c.weight_kind, c.d_edge_w, c.len_in, c.d_in, c.d_agg, c.flags & GAIB_ACCUMULATE));
  if (!dual) return trailing_gemm(ctx, g, c, c.d_agg, c.d_W, 0);
  GAIB_TRY(gaib_sgemm_ex(ctx, 0, c.transW, g->nv, c.len_out, c.len_in, c.d_agg, c.d_W, 0, c.d_out));
  return trailing_gemm(ctx, g, c, c.d_rows2, c.d_W2, GAIB_ACCUMULATE);
}

static int spmm_gemm_run(gaib_ctx* ctx, gaib_graph* g, const GemmCall& c) {
  GemmRoute r;
  GAIB_TRY(gemm_route(ctx, g, c, &r));
  switch (r.kind) {
    case ROUTE_FUSED: return run_fused(ctx, g, c, r.form);
    case ROUTE_FUSED_THEN_GEMM: {  // the neighbour product rides on the aggregation, the self term follows and applies the activation
      GemmCall n = c;
      n.d_rows2 = n.d_W2 = nullptr;
      n.flags &= ~GAIB_RELU;
      GAIB_TRY(run_fused(ctx, g, n, r.form));
      return trailing_gemm(ctx, g, c, c.d_rows2, c.d_W2, GAIB_ACCUMULATE);
    }
    case ROUTE_KSLABS: return run_kslabs(ctx, g, c, r.form);
    case ROUTE_UNFUSED: return run_unfused(ctx, g, c);
    default: return GAIB_OK;  // ROUTE_NONE (a refusal has returned its code above)
  }
}

extern "C" int gaib_spmm_gemm(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w,
                              int len_in, const float* d_in, float* d_agg, const float* d_W, int transW,
                              int len_out, float* d_out, int flags) {
  return spmm_gemm_run(ctx, g, GemmCall{weight_kind, d_edge_w, len_in, d_in, d_agg, d_W, transW, nullptr, nullptr, len_out, d_out, flags});
}

extern "C" int gaib_spmm_gemm2(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w,
                               int len_in, const float* d_in, float* d_agg, const float* d_W, int transW,
                               const float* d_rows2, const float* d_W2, int len_out, float* d_out, int flags) {
  GAIB_CHECK(d_rows2 && d_W2, "gaib_spmm_gemm2: NULL second operand");
  return spmm_gemm_run(ctx, g, GemmCall{weight_kind, d_edge_w, len_in, d_in, d_agg, d_W, transW, d_rows2, d_W2, len_out, d_out, flags});
}

// Would gaib_spmm_gemm_zs / gaib_spmm_gemm2_zs (d_rows2 != NULL) take this call?  GAIB_OK or GAIB_ERR_UNSUPPORTED from the route
// function alone: nothing is launched, nothing is read through the pointers -- a caller asks BEFORE it packs.
extern "C" int gaib_spmm_gemm_zs_route(gaib_ctx* ctx, gaib_graph* g, int weight_kind, int len_in, const float* d_in, const void* d_zs,
                                       float* d_agg, const float* d_rows2, int len_out, float* d_out) {
  GAIB_CHECK(d_zs, "gaib_spmm_gemm_zs_route: NULL packed table");
  GemmCall c{weight_kind, nullptr, len_in, d_in, d_agg, d_in, 1, d_rows2, d_rows2 ? d_in : nullptr, len_out, d_out, 0};
  c.d_zs = d_zs;
  GemmRoute r;
  return gemm_route(ctx, g, c, &r);
}

// agg = A.in ; out = act(agg . op(W) [+ rows2 . op(W2)]) gathering from the zero-suppressed image d_zs of d_in (gaib_pack_zs at 128
// columns, gaib_pack_zs_wide at 256): three lines per gathered (half) row instead of four, d_agg (unless scratch) and d_out
// bit-identical to gaib_spmm_gemm(2) on d_in.
extern "C" int gaib_spmm_gemm_zs(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in,
                                 const float* d_in, const void* d_zs, float* d_agg, const float* d_W, int transW, int len_out,
                                 float* d_out, int flags) {
  GAIB_CHECK(d_zs, "gaib_spmm_gemm_zs: NULL packed table");
  GAIB_CHECK(!(flags & GAIB_OVERLAPS_TRANSFER), "gaib_spmm_gemm_zs: GAIB_OVERLAPS_TRANSFER belongs to partitioned runs, which gather dense tables");
  GemmCall c{weight_kind, d_edge_w, len_in, d_in, d_agg, d_W, transW, nullptr, nullptr, len_out, d_out, flags};
  c.d_zs = d_zs;
  return spmm_gemm_run(ctx, g, c);
}

extern "C" int gaib_spmm_gemm2_zs(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in,
                                  const float* d_in, const void* d_zs, float* d_agg, const float* d_W, int transW,
                                  const float* d_rows2, const float* d_W2, int len_out, float* d_out, int flags) {
  GAIB_CHECK(d_zs, "gaib_spmm_gemm2_zs: NULL packed table");
  GAIB_CHECK(d_rows2 && d_W2, "gaib_spmm_gemm2_zs: NULL second operand");
  GAIB_CHECK(!(flags & GAIB_OVERLAPS_TRANSFER), "gaib_spmm_gemm2_zs: GAIB_OVERLAPS_TRANSFER belongs to partitioned runs, which gather dense tables");
  GemmCall c{weight_kind, d_edge_w, len_in, d_in, d_agg, d_W, transW, d_rows2, d_W2, len_out, d_out, flags};
  c.d_zs = d_zs;
  return spmm_gemm_run(ctx, g, c);
}

extern "C" int gaib_spmm_gemm_2t(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in,
                                 const float* d_in, const float* d_in2, int64_t n_first, float* d_agg, const float* d_W,
                                 int transW, const float* d_rows2, const float* d_W2, int len_out, float* d_out, int flags) {
  GAIB_CHECK(ctx && g, "gaib_spmm_gemm_2t: NULL ctx/graph");
  GAIB_CHECK(d_in2 || n_first >= g->nc || g->nv == 0 || g->ne == 0, "gaib_spmm_gemm_2t: NULL second table with columns beyond n_first");
  GAIB_CHECK(!d_in2 || (d_in2 != d_agg && d_in2 != d_out), "gaib_spmm_gemm_2t: buffers must not alias");
  GemmCall c{weight_kind, d_edge_w, len_in, d_in, d_agg, d_W, transW, d_rows2, d_W2, len_out, d_out, flags};
  c.d_in2 = d_in2;
  c.n_first = n_first;
  return spmm_gemm_run(ctx, g, c);
}

extern "C" int gaib_spmm_mh(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w,
                            int heads, int len, const float* d_in, float* d_out, int flags) {
  GAIB_CHECK(heads >= 1 && len % heads == 0, "gaib_spmm_mh: heads (%d) must divide len (%d)", heads, len);
  GAIB_CHECK(heads == 1 || weight_kind == GAIB_W_EDGE || weight_kind == GAIB_W_EDGE_T,
             "gaib_spmm_mh: per-head weights need GAIB_W_EDGE or GAIB_W_EDGE_T");
  return spmm_impl(ctx, g, weight_kind, d_edge_w, len, d_in, d_out, flags, heads);
}

// ---- bf16 feature tables ------------------------------------------------------------------------------------------------
// out[i,:] (+)= sum_e w_e * widen(in[col_e,:]) with in in bf16 (raw bits), out in fp32.  The kernels are the fp32 ones with
// a bf16 gather (RowGather<.., E = uint16_t>): the same weights, the same CSR order with separate multiply and add, the same
// row classes (heavy threshold, 16-wave split, LDS combine in wave order) and the same choice of the ordered-chunk form for
// dense graphs -- so the result is bit-identical to gaib_spmm_ex on the table widened to fp32.  Only the lane layout
// differs: a row needs half the bytes, so a lane takes twice the elements for the same load width.
namespace {

template <int WMODE>
int dispatch_bf16(gaib_ctx* ctx, gaib_graph* g, const SpmmArgs& a0, int len) {
  typedef uint16_t bf16_t;
  // widest vector the row length, the row stride and the base pointers allow: VEC elements = 2 VEC bytes per gather, 4 VEC bytes
  // per store (a lane never reaches past column len: the columns behind it in a strided table are not read)
  const uintptr_t ai = (uintptr_t)a0.in, ao = (uintptr_t)a0.out;
  int vmax = 1;
  for (int v = 8; v > 1; v >>= 1)
    if (len % v == 0 && a0.ld % v == 0 && (ai & (2 * v - 1)) == 0 && (ao & ((v >= 4 ? 16 : 4 * v) - 1)) == 0) {
      vmax = v;
      break;
    }
  // option spmm_bf16_layout (A/B of the lane layout; LEDGER): 0 = one row per wave, the narrowest lane that covers a row in
  // one pass (128 columns: 4-B lanes); 4 / 8 = sub-wave rows of 4 / 8 elements per lane (128 columns: 2 / 4 rows per wave)
  const int layout = ctx->spmm_bf16_layout;
  if ((layout == 4 || layout == 8) && vmax >= layout && (len + layout - 1) / layout <= 32) {
    const int lanes = (len + layout - 1) / layout;
    if (layout == 8) {
      if (lanes <= 1) return launch_sub<8, 1, WMODE, bf16_t>(ctx, g, a0);
      if (lanes <= 2) return launch_sub<8, 2, WMODE, bf16_t>(ctx, g, a0);
      if (lanes <= 4) return launch_sub<8, 4, WMODE, bf16_t>(ctx, g, a0);
      if (lanes <= 8) return launch_sub<8, 8, WMODE, bf16_t>(ctx, g, a0);
      if (lanes <= 16) return launch_sub<8, 16, WMODE, bf16_t>(ctx, g, a0);
      return launch_sub<8, 32, WMODE, bf16_t>(ctx, g, a0);
    }
    if (lanes <= 1) return launch_sub<4, 1, WMODE, bf16_t>(ctx, g, a0);
    if (lanes <= 2) return launch_sub<4, 2, WMODE, bf16_t>(ctx, g, a0);
    if (lanes <= 4) return launch_sub<4, 4, WMODE, bf16_t>(ctx, g, a0);
    if (lanes <= 8) return launch_sub<4, 8, WMODE, bf16_t>(ctx, g, a0);
    if (lanes <= 16) return launch_sub<4, 16, WMODE, bf16_t>(ctx, g, a0);
    return launch_sub<4, 32, WMODE, bf16_t>(ctx, g, a0);
  }
  int vec = vmax;
  for (int v = 1; v < vmax; v <<= 1)
    if ((len + v - 1) / v <= 64) {
      vec = v;
      break;
    }
  // one launch covers up to 256 lanes of <= 2 elements, 128 of 4 or 64 of 8 (as in fp32, 16 accumulators per lane next to
  // the gathers spill); wider rows in column slabs, each walking the edge list again
  const int slab = vec >= 4 ? 512 : 256 * vec;
  for (int c0 = 0; c0 < len; c0 += slab) {
    SpmmArgs a = a0;
    a.in = reinterpret_cast<const float*>(reinterpret_cast<const bf16_t*>(a0.in) + c0);
    a.out = a0.out + c0;
    if (a.in_bytes) a.in_bytes -= (uint32_t)(2 * c0);
    a.ncols = (len - c0 < slab) ? (len - c0) : slab;
    const int lanes = (a.ncols + vec - 1) / vec;
    const int ct = lanes <= 64 ? 1 : (lanes <= 128 ? 2 : 4);
    int rc;
    if (vec == 8) rc = launch_w64<8, 1, WMODE, bf16_t>(ctx, g, a);
    else if (vec == 4) rc = ct == 1 ? launch_w64<4, 1, WMODE, bf16_t>(ctx, g, a) : launch_w64<4, 2, WMODE, bf16_t>(ctx, g, a);
    else if (vec == 2) rc = ct == 1 ? launch_w64<2, 1, WMODE, bf16_t>(ctx, g, a)
                                    : (ct == 2 ? launch_w64<2, 2, WMODE, bf16_t>(ctx, g, a) : launch_w64<2, 4, WMODE, bf16_t>(ctx, g, a));
    else rc = ct == 1 ? launch_w64<1, 1, WMODE, bf16_t>(ctx, g, a)
                      : (ct == 2 ? launch_w64<1, 2, WMODE, bf16_t>(ctx, g, a) : launch_w64<1, 4, WMODE, bf16_t>(ctx, g, a));
    if (rc != GAIB_OK) return rc;
  }
  return GAIB_OK;
}

}  // namespace

// ld: the table's row stride in elements -- len (dense), or a multiple of 4 above it (rows keep the table's 8-B alignment).  It
// enters the gather addresses only: every route decision below is made on len, so a strided call sums in the dense call's order.
extern "C" int gaib_spmm_bf16_ld(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len, int64_t ld,
                                 const uint16_t* d_in, float* d_out, int flags) {
  GAIB_CHECK(ctx && g, "gaib_spmm_bf16: NULL ctx/graph");
  GAIB_CHECK(len >= 0, "gaib_spmm_bf16: len < 0");
  GAIB_CHECK(ld == len || (ld > len && ld % 4 == 0), "gaib_spmm_bf16_ld: row stride ld (%lld) must be len (%d) or a multiple of 4 above it",
             (long long)ld, len);
  GAIB_CHECK((flags & ~(GAIB_ACCUMULATE | GAIB_RELU)) == 0, "gaib_spmm_bf16: unsupported flags %d", flags);
  GAIB_CHECK(ctx->device == g->device, "gaib_spmm_bf16: graph lives on device %d, ctx on %d", g->device, ctx->device);
  if (g->row_map) {
    gaib_set_error("gaib_spmm_bf16: a row class of a partition (graph with a row map) is not supported: fp32 tables only");
    return GAIB_ERR_UNSUPPORTED;
  }
  if (len == 0 || g->nv == 0) return GAIB_OK;
  GAIB_CHECK(d_in && d_out, "gaib_spmm_bf16: NULL feature pointer");
  GAIB_CHECK((const void*)d_in != (const void*)d_out, "gaib_spmm_bf16: in and out must not alias");
  SpmmArgs a;
  int wmode = 0;
  GAIB_TRY(spmm_setup(ctx, g, weight_kind, d_edge_w, len, reinterpret_cast<const float*>(d_in), d_out, flags, 1, &a, &wmode,
                      nullptr, 0, true, ld));
  // the fp32 path's choice of the ordered-chunk form, made on what IT would see (the row stride of its possibly re-strided
  // table; 16-B aligned rows) -- the same graph and len take the same summation order
  const int64_t ld32 = pad_stride_floats(ctx, g, len, false) > 0 ? pad_stride_floats(ctx, g, len, false) : len;
  const bool chunk_shape = len % 4 == 0 && len <= 256 && g->ne > 0 && (((uintptr_t)d_in & 7) == 0) &&
                           (((uintptr_t)d_out & 15) == 0);
  if (chunk_shape && (ctx->spmm_chunked == 1 || (ctx->spmm_chunked < 0 && chunk_rule(ctx, g, ld32)))) {
    switch (wmode) {
      case 0: return launch_chunked<0, uint16_t>(ctx, g, a);
      case 1: return launch_chunked<1, uint16_t>(ctx, g, a);
      default: return launch_chunked<2, uint16_t>(ctx, g, a);
    }
  }
  switch (wmode) {
    case 0: return dispatch_bf16<0>(ctx, g, a, len);
    case 1: return dispatch_bf16<1>(ctx, g, a, len);
    default: return dispatch_bf16<2>(ctx, g, a, len);
  }
}

extern "C" int gaib_spmm_bf16(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len,
                              const uint16_t* d_in, float* d_out, int flags) {
  return gaib_spmm_bf16_ld(ctx, g, weight_kind, d_edge_w, len, len, d_in, d_out, flags);
}

// agg = A.widen(in) ; out = act(agg . op(W) [+ rows2 . op(W2)]) with `in` in bf16 (raw bits), everything else fp32: the route
// gaib_spmm_gemm(2) takes on the widened table, run with the bf16 gather -- d_agg (unless scratch) and d_out bit-identical to
// that call, for d_in aligned to 8 B and d_agg to 16.
// ld: the table's row stride in elements (see gaib_spmm_bf16_ld); the route is chosen on len_in, as for the dense table.
static int spmm_gemm_bf16_entry(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, int64_t ld,
                                const uint16_t* d_in, float* d_agg, const float* d_W, int transW, const float* d_rows2,
                                const float* d_W2, int len_out, float* d_out, int flags) {
  GAIB_CHECK(ctx && g, "gaib_spmm_gemm_bf16: NULL ctx/graph");
  GAIB_CHECK(ld == len_in || (ld > len_in && ld % 4 == 0),
             "gaib_spmm_gemm_bf16_ld: row stride ld (%lld) must be len_in (%d) or a multiple of 4 above it", (long long)ld, len_in);
  GAIB_CHECK(!(flags & GAIB_OVERLAPS_TRANSFER), "gaib_spmm_gemm_bf16: GAIB_OVERLAPS_TRANSFER belongs to partitioned runs, which "
                                                "aggregate fp32 tables");
  if (g->row_map) {
    gaib_set_error("gaib_spmm_gemm_bf16: a row class of a partition (graph with a row map) is not supported: fp32 tables only");
    return GAIB_ERR_UNSUPPORTED;
  }
  GemmCall c{weight_kind, d_edge_w, len_in, reinterpret_cast<const float*>(d_in), d_agg, d_W, transW, d_rows2, d_W2, len_out, d_out, flags};
  c.bf16 = true;
  c.ld = ld;
  return spmm_gemm_run(ctx, g, c);
}

extern "C" int gaib_spmm_gemm_bf16(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in,
                                   const uint16_t* d_in, float* d_agg, const float* d_W, int transW, int len_out, float* d_out,
                                   int flags) {
  return spmm_gemm_bf16_entry(ctx, g, weight_kind, d_edge_w, len_in, len_in, d_in, d_agg, d_W, transW, nullptr, nullptr, len_out,
                              d_out, flags);
}

extern "C" int gaib_spmm_gemm_bf16_ld(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, int64_t ld,
                                      const uint16_t* d_in, float* d_agg, const float* d_W, int transW, int len_out, float* d_out,
                                      int flags) {
  return spmm_gemm_bf16_entry(ctx, g, weight_kind, d_edge_w, len_in, ld, d_in, d_agg, d_W, transW, nullptr, nullptr, len_out,
                              d_out, flags);
}

extern "C" int gaib_spmm_gemm2_bf16_ld(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, int64_t ld,
                                       const uint16_t* d_in, float* d_agg, const float* d_W, int transW, const float* d_rows2,
                                       const float* d_W2, int len_out, float* d_out, int flags) {
  GAIB_CHECK(d_rows2 && d_W2, "gaib_spmm_gemm2_bf16_ld: NULL second operand");
  return spmm_gemm_bf16_entry(ctx, g, weight_kind, d_edge_w, len_in, ld, d_in, d_agg, d_W, transW, d_rows2, d_W2, len_out, d_out,
                              flags);
}

extern "C" int gaib_spmm_gemm2_bf16(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in,
                                    const uint16_t* d_in, float* d_agg, const float* d_W, int transW, const float* d_rows2,
                                    const float* d_W2, int len_out, float* d_out, int flags) {
  GAIB_CHECK(d_rows2 && d_W2, "gaib_spmm_gemm2_bf16: NULL second operand");
  return spmm_gemm_bf16_entry(ctx, g, weight_kind, d_edge_w, len_in, len_in, d_in, d_agg, d_W, transW, d_rows2, d_W2, len_out,
                              d_out, flags);
}

// ---- bf16 feature tables on the row classes of a vertex-range partition (spmm_part_bf16.hip) ----------------------------------
// gaib_spmm_ex (d_in2 == NULL; n_first is then ignored) / gaib_spmm_2t with the table(s) in bf16: graphs with or without a row map,
// one table or [owned | halo].  A whole
// graph over one table is gaib_spmm_bf16's call; a row class takes the class kernels' route (no ordered chunks, no re-strided
// copy -- as gaib_spmm_ex on a class graph) with the bf16 gather, so the result is bit-identical to the fp32 call on the widened
// tables.
extern "C" int gaib_spmm_part_bf16(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len,
                                   const uint16_t* d_in, const uint16_t* d_in2, int64_t n_first, float* d_out, int flags) {
  GAIB_CHECK(ctx && g, "gaib_spmm_part_bf16: NULL ctx/graph");
  if (!g->row_map && !d_in2) {
    return gaib_spmm_bf16(ctx, g, weight_kind, d_edge_w, len, d_in, d_out, flags);
  }
  GAIB_CHECK(len >= 0, "gaib_spmm_part_bf16: len < 0");
  GAIB_CHECK((flags & ~(GAIB_ACCUMULATE | GAIB_RELU)) == 0, "gaib_spmm_part_bf16: unsupported flags %d", flags);
  GAIB_CHECK(ctx->device == g->device, "gaib_spmm_part_bf16: graph lives on device %d, ctx on %d", g->device, ctx->device);
  if (len == 0 || g->nv == 0) return GAIB_OK;
  GAIB_CHECK(d_in && d_out, "gaib_spmm_part_bf16: NULL feature pointer");
  GAIB_CHECK((const void*)d_in != (const void*)d_out && (const void*)d_in2 != (const void*)d_out,
             "gaib_spmm_part_bf16: in / in2 and out must not alias");
  SpmmArgs a;
  int wmode = 0;
  GAIB_TRY(spmm_setup(ctx, g, weight_kind, d_edge_w, len, reinterpret_cast<const float*>(d_in), d_out, flags, 1, &a, &wmode,
                      reinterpret_cast<const float*>(d_in2), n_first, true));
  GAIB_CHECK(wmode <= 1, "gaib_spmm_part_bf16: a row class of a partition aggregates with GAIB_W_GCN / _MEAN / _MEAN_T / single-head "
                         "_EDGE weights (got kind %d)", weight_kind);
  return gaib_spmm_part_plain_bf16(ctx, g, a, wmode, len);
}

// gaib_spmm_gemm_2t with the table(s) in bf16 (d_rows2 / d_W2: both or NULL; d_in2 may be NULL): the route of the fp32 call on the
// widened tables -- a row class runs the fused class kernels or is refused where the fp32 call refuses it, a whole graph takes
// gaib_spmm_gemm(2)_bf16's routes -- with every flag of gaib_spmm_gemm_2t, GAIB_OVERLAPS_TRANSFER included.
extern "C" int gaib_spmm_gemm_part_bf16(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in,
                                        const uint16_t* d_in, const uint16_t* d_in2, int64_t n_first, float* d_agg, const float* d_W,
                                        int transW, const float* d_rows2, const float* d_W2, int len_out, float* d_out, int flags) {
  GAIB_CHECK(ctx && g, "gaib_spmm_gemm_part_bf16: NULL ctx/graph");
  GAIB_CHECK(!d_in2 || ((const void*)d_in2 != (const void*)d_agg && (const void*)d_in2 != (const void*)d_out),
             "gaib_spmm_gemm_part_bf16: buffers must not alias");
  GemmCall c{weight_kind, d_edge_w, len_in, reinterpret_cast<const float*>(d_in), d_agg, d_W, transW, d_rows2, d_W2, len_out, d_out, flags};
  c.d_in2 = reinterpret_cast<const float*>(d_in2);
  c.n_first = n_first;
  c.bf16 = true;
  return spmm_gemm_run(ctx, g, c);
}

// ---- fp8 feature tables with per-row scales (the kernels: spmm_fp8.hip, spmm_gemm_fp8.hip) ------------------------
// The table is e4m3 "fn" bytes [nc x ld] (ld = the row stride in bytes) with a power-of-two scale per row; row r stands for
// f32(q[r][:]) * scale[r], both steps exact.  The kernels are the fp32 ones with an fp8 gather (RowGather<.., E = fp8_t>) and the
// scale of an edge's column folded into its weight (spmm_core.h): the same CSR order with separate multiply and add, the same
// heavy threshold and 16-wave LDS combine, the same choice of the ordered-chunk form -- made on what the fp32 call would see --,
// so the result is bit-identical to gaib_spmm_ex / gaib_spmm_gemm(2) on the widened table while w_e * scale and the products
// stay normal numbers.
extern "C" int gaib_fp8_row_stride(int len, int64_t* ld) {
  GAIB_CHECK(ld, "gaib_fp8_row_stride: NULL argument");
  GAIB_CHECK(len >= 0, "gaib_fp8_row_stride: len < 0");
  if (len % 128 == 0) *ld = len;
  else if (len <= 128) {
    int64_t p = 4;
    while (p < len) p <<= 1;
    *ld = p;
  } else *ld = ((int64_t)len + 127) / 128 * 128;
  return GAIB_OK;
}

// what every fp8 aggregation call checks before it touches anything; GAIB_ERR_UNSUPPORTED for what the fp8 gather does not have
static int fp8_table_check(const char* who, const gaib_graph* g, int len, int64_t ld, const uint8_t* d_q) {
  GAIB_CHECK(len >= 0, "%s: len < 0", who);
  GAIB_CHECK(ld >= len && ld % 4 == 0, "%s: row stride ld (%lld bytes) must be a multiple of 4 not below len (%d): gaib_fp8_row_stride",
             who, (long long)ld, len);
  if (g->row_map) {
    gaib_set_error("%s: a row class of a partition (graph with a row map) is not supported: fp32 or bf16 tables only", who);
    return GAIB_ERR_UNSUPPORTED;
  }
  if (g->nc * ld >= ((int64_t)1 << 32)) {
    gaib_set_error("%s: an fp8 table of 4 GB or more (%lld rows of %lld bytes) is not supported: buffer addressing only", who,
                   (long long)g->nc, (long long)ld);
    return GAIB_ERR_UNSUPPORTED;
  }
  if (((uintptr_t)d_q & 15) != 0) {
    gaib_set_error("%s: the fp8 table must start on a 16-byte boundary", who);
    return GAIB_ERR_UNSUPPORTED;
  }
  return GAIB_OK;
}

extern "C" int gaib_spmm_fp8(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len, int64_t ld,
                             const uint8_t* d_q, const float* d_scale, float* d_out, int flags) {
  GAIB_CHECK(ctx && g, "gaib_spmm_fp8: NULL ctx/graph");
  GAIB_CHECK((flags & ~(GAIB_ACCUMULATE | GAIB_RELU)) == 0, "gaib_spmm_fp8: unsupported flags %d", flags);
  GAIB_CHECK(ctx->device == g->device, "gaib_spmm_fp8: graph lives on device %d, ctx on %d", g->device, ctx->device);
  GAIB_TRY(fp8_table_check("gaib_spmm_fp8", g, len, ld, d_q));
  if (len == 0 || g->nv == 0) return GAIB_OK;
  GAIB_CHECK(d_q && d_scale && d_out, "gaib_spmm_fp8: NULL table, scale or output pointer");
  GAIB_CHECK((const void*)d_q != (const void*)d_out && (const void*)d_scale != (const void*)d_out, "gaib_spmm_fp8: in and out must not alias");
  SpmmArgs a;
  int wmode = 0;
  GAIB_TRY(spmm_setup(ctx, g, weight_kind, d_edge_w, len, reinterpret_cast<const float*>(d_q), d_out, flags, 1, &a, &wmode, nullptr, 0,
                      false, ld, true));
  a.in2 = d_scale;
  // the fp32 path's choice of the ordered-chunk form, made on what IT would see (as gaib_spmm_bf16_ld): the widened table is
  // 16-B aligned wherever this one is 4-B aligned
  const int64_t ld32 = pad_stride_floats(ctx, g, len, false) > 0 ? pad_stride_floats(ctx, g, len, false) : len;
  const bool chunk_shape = len % 4 == 0 && len <= 256 && g->ne > 0 && (((uintptr_t)d_out & 15) == 0);
  if (chunk_shape && (ctx->spmm_chunked == 1 || (ctx->spmm_chunked < 0 && chunk_rule(ctx, g, ld32)))) {
    switch (wmode) {
      case 0: return launch_chunked<0, fp8_t>(ctx, g, a);
      case 1: return launch_chunked<1, fp8_t>(ctx, g, a);
      default: return launch_chunked<2, fp8_t>(ctx, g, a);
    }
  }
  return gaib_spmm_plain_fp8(ctx, g, a, wmode, len);
}

// agg = A.widen(q, scale) ; out = act(agg . op(W) [+ rows2 . op(W2)]): the route gaib_spmm_gemm(2) takes on the widened table
// (gemm_route: every test on the fp32 sizes), run with the fp8 gather.
static int spmm_gemm_fp8_entry(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, int64_t ld,
                               const uint8_t* d_q, const float* d_scale, float* d_agg, const float* d_W, int transW,
                               const float* d_rows2, const float* d_W2, int len_out, float* d_out, int flags) {
  GAIB_CHECK(ctx && g, "gaib_spmm_gemm_fp8: NULL ctx/graph");
  GAIB_CHECK(!(flags & GAIB_OVERLAPS_TRANSFER), "gaib_spmm_gemm_fp8: GAIB_OVERLAPS_TRANSFER belongs to partitioned runs, which "
                                                "aggregate fp32 or bf16 tables");
  GAIB_TRY(fp8_table_check("gaib_spmm_gemm_fp8", g, len_in, ld, d_q));
  GAIB_CHECK(g->nv == 0 || len_out == 0 || d_scale, "gaib_spmm_gemm_fp8: NULL scale pointer");
  GAIB_CHECK((const void*)d_scale != (const void*)d_agg && (const void*)d_scale != (const void*)d_out, "gaib_spmm_gemm_fp8: buffers must not alias");
  GemmCall c{weight_kind, d_edge_w, len_in, reinterpret_cast<const float*>(d_q), d_agg, d_W, transW, d_rows2, d_W2, len_out, d_out, flags};
  c.fp8 = true;
  c.ld = ld;
  c.d_scale = d_scale;
  return spmm_gemm_run(ctx, g, c);
}

extern "C" int gaib_spmm_gemm_fp8(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, int64_t ld,
                                  const uint8_t* d_q, const float* d_scale, float* d_agg, const float* d_W, int transW, int len_out,
                                  float* d_out, int flags) {
  return spmm_gemm_fp8_entry(ctx, g, weight_kind, d_edge_w, len_in, ld, d_q, d_scale, d_agg, d_W, transW, nullptr, nullptr, len_out,
                             d_out, flags);
}

extern "C" int gaib_spmm_gemm2_fp8(gaib_ctx* ctx, gaib_graph* g, int weight_kind, const float* d_edge_w, int len_in, int64_t ld,
                                   const uint8_t* d_q, const float* d_scale, float* d_agg, const float* d_W, int transW,
                                   const float* d_rows2, const float* d_W2, int len_out, float* d_out, int flags) {
  GAIB_CHECK(d_rows2 && d_W2, "gaib_spmm_gemm2_fp8: NULL second operand");
  return spmm_gemm_fp8_entry(ctx, g, weight_kind, d_edge_w, len_in, ld, d_q, d_scale, d_agg, d_W, transW, d_rows2, d_W2, len_out, d_out,
                             flags);
}
