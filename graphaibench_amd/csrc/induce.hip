// induce.hip -- the subgraph a vertex set induces on a graph in HBM, built on the device: what Sampler::generateSubgraph
// (src/gnn/sampler.cpp, GAIB_INDUCE_RELABEL) and LearningGraph::generate_masked_graph (GAIB_INDUCE_KEEP_IDS) build on the
// host, array for array.  Sibling of gaib_graph_add_selfloop / gaib_graph_reorder (graph.hip).  DESIGN.md 10.
//
// Membership and rank come from a bitmap of nv bits plus one uint32 prefix count per 64-bit word, cached on the graph
// (gaib_graph::induce_bits / induce_prefix):  rank(v) = prefix[v >> 6] + popcll(word & ((1 << (v & 63)) - 1)).  At the
// products size that is 306 KB + 153 KB -- resident in every XCD's 4 MiB L2, where a 4-byte relabel table (10 MB) is not.
// Two passes over the KEPT rows only: a wave walks a row in chunks of 64 edges (coalesced column ids, bitmap word gather,
// __ballot); the count pass sums popcll(ballot), the fill pass writes at base + popcll(ballot & lanes below), so a row's
// surviving edges keep their order by construction.  Integer atomics only (64-bit OR into the bitmap: order-free).
#include <hipcub/hipcub.hpp>

#include "common.h"

namespace {

// bit v for every kept vertex; d_rows[i] = kept[i] widened.  A list that is not strictly ascending, or an id >= nv, raises
// *bad -- the id is compared, never used as an address.
__global__ void induce_mark_kernel(int64_t n_kept, const uint32_t* kept, int64_t nv, unsigned long long* bits,
                                   int64_t* d_rows, int64_t* bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_kept) return;
  const uint32_t v = kept[i];
  if ((int64_t)v >= nv || (i > 0 && kept[i - 1] >= v)) {
    *bad = 1;  // (every writer writes the same value)
    return;
  }
  atomicOr(&bits[v >> 6], 1ull << (v & 63));
  if (d_rows) d_rows[i] = (int64_t)v;
}

// per-word popcounts, entry nw = 0: the input of the exclusive scan that gives the prefix directory [nw + 1]
__global__ void induce_popc_kernel(int64_t nw, const unsigned long long* bits, uint32_t* cnt) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < nw) cnt[w] = (uint32_t)__popcll(bits[w]);
  else if (w == nw) cnt[w] = 0u;
}

__device__ __forceinline__ bool bit_of(const unsigned long long* bits, uint32_t v) { return (bits[v >> 6] >> (v & 63)) & 1ull; }

// One wave per output row.  RELABEL: output row r is row kept[r] of g.  KEEP_IDS: output row r is row r, empty -- without
// reading its edges -- where r's own bit is clear.
// FILL = false: cnt[r] = surviving edges of the row (cnt[rows] = 0).  FILL = true: the surviving column ids (RELABEL: their
// ranks) to col_out[rowptr_out[r] ...) in input order.
template <bool FILL, bool RELABEL>
__global__ __launch_bounds__(256) void induce_rows_kernel(int64_t rows, int64_t nv, const uint32_t* kept, const int64_t* rowptr,
                                                          const uint32_t* col, const unsigned long long* bits,
                                                          const uint32_t* prefix, int64_t* cnt, const int64_t* rowptr_out,
                                                          uint32_t* col_out) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r > rows || (FILL && r == rows)) return;
  if (r == rows) {
    if (lane == 0) cnt[rows] = 0;
    return;
  }
  int64_t src = r;
  bool live = true;
  if (RELABEL) {
    src = (int64_t)kept[r];
    live = src < nv;  // (a refused list: the count pass runs before the flag is read back; no address from a bad id)
  } else {
    live = bit_of(bits, (uint32_t)r);
  }
  int64_t e0 = 0, e1 = 0;
  if (live) {
    e0 = rowptr[src];
    e1 = rowptr[src + 1];
  }
  int64_t base = FILL ? rowptr_out[r] : 0;  // wave-uniform: carried in scalar registers
  for (int64_t e = e0; e < e1; e += 64) {
    const bool valid = e + lane < e1;
    const uint32_t c = valid ? col[e + lane] : 0u;
    const unsigned long long word = valid ? bits[c >> 6] : 0ull;
    const bool keep = (word >> (c & 63)) & 1ull;
    const unsigned long long ballot = __ballot(keep);
    if (FILL && keep) {
      const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
      col_out[base + below] = RELABEL ? prefix[c >> 6] + (uint32_t)__popcll(word & ((1ull << (c & 63)) - 1ull)) : c;
    }
    base += __popcll(ballot);
  }
  if (!FILL && lane == 0) cnt[r] = base;
}

// out[k, :] = in[idx[k], :] for rows of `width` bytes: one thread per byte (label rows: 1 byte single-class, one byte per class
// multi-label), no alignment asked of either side
__global__ void gather_rows_u8_kernel(int64_t total, int width, const int64_t* idx, const uint8_t* in, uint8_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = i / width;
    out[i] = in[idx[k] * width + (i - k * width)];
  }
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

int gaib_graph_ensure_induce(gaib_ctx* ctx, gaib_graph* g) {
  if (g->induce_bits) return GAIB_OK;
  GAIB_NOT_WHILE_CAPTURING(ctx, "building the graph's membership bitmap");
  const int64_t nw = cdiv64(g->nv, 64);
  unsigned long long* bits = nullptr;
  GAIB_HIP(hipMalloc(&bits, sizeof(unsigned long long) * (size_t)(nw > 0 ? nw : 1)));
  hipError_t e = hipMalloc(&g->induce_prefix, sizeof(uint32_t) * (size_t)(nw + 1));
  if (e != hipSuccess) {
    (void)hipFree(bits);
    g->induce_prefix = nullptr;
    gaib_set_error("membership bitmap: hipMalloc: %s", hipGetErrorString(e));
    return GAIB_ERR_NOMEM;
  }
  g->induce_bits = bits;
  g->dev_bytes += sizeof(unsigned long long) * nw + sizeof(uint32_t) * (nw + 1);
  return GAIB_OK;
}

extern "C" int gaib_graph_induce(gaib_ctx* ctx, gaib_graph* g, int64_t n_kept, const uint32_t* kept, int kept_on_device,
                                 int mode, gaib_graph** out, int64_t* d_rows_out) {
  GAIB_CHECK(ctx && g && out && (kept || n_kept == 0), "gaib_graph_induce: NULL argument");
  GAIB_CHECK(mode == GAIB_INDUCE_RELABEL || mode == GAIB_INDUCE_KEEP_IDS, "gaib_graph_induce: unknown mode %d", mode);
  if (g->nc != g->nv) {
    gaib_set_error("gaib_graph_induce: square graphs only (this one has %lld rows and %lld columns)", (long long)g->nv,
                   (long long)g->nc);
    return GAIB_ERR_UNSUPPORTED;
  }
  GAIB_CHECK(!g->row_map, "gaib_graph_induce: not on a class graph");
  GAIB_CHECK(n_kept >= 0 && n_kept <= g->nv, "gaib_graph_induce: %lld kept vertices of %lld (strictly ascending ids < nv)",
             (long long)n_kept, (long long)g->nv);
  GAIB_NOT_WHILE_CAPTURING(ctx, "gaib_graph_induce");
  GAIB_HIP(hipSetDevice(ctx->device));
  *out = nullptr;
  hipStream_t st = ctx->stream;
  const bool relabel = mode == GAIB_INDUCE_RELABEL;
  const int64_t nv = g->nv, nw = cdiv64(nv, 64), rows = relabel ? n_kept : nv;
  GAIB_TRY(gaib_graph_ensure_induce(ctx, g));
  unsigned long long* bits = (unsigned long long*)g->induce_bits;

  // scratch, all in the context's workspace: [kept copy] | word counts [nw + 1] | row counts [rows + 1] |
  // row pointers [rows + 1] + the flag | the scans' temporary storage
  size_t scan_w = 0, scan_r = 0;
  GAIB_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_w, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(nw + 1), st));
  GAIB_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_r, (int64_t*)nullptr, (int64_t*)nullptr, (int)(rows + 1), st));
  const size_t scan_bytes = scan_w > scan_r ? scan_w : scan_r;
  const size_t o_kept = 0, o_wcnt = o_kept + (kept_on_device ? 0 : up256(sizeof(uint32_t) * n_kept)),
               o_cnt = o_wcnt + up256(sizeof(uint32_t) * (nw + 1)), o_rp = o_cnt + up256(sizeof(int64_t) * (rows + 1)),
               o_scan = o_rp + up256(sizeof(int64_t) * (rows + 2)), ws_need = o_scan + up256(scan_bytes);
  GAIB_TRY(gaib_ws_reserve(ctx, ws_need));
  char* ws = (char*)ctx->ws;
  const uint32_t* d_kept = kept;
  if (!kept_on_device && n_kept > 0) {
    GAIB_HIP(hipMemcpyAsync(ws + o_kept, kept, sizeof(uint32_t) * n_kept, hipMemcpyHostToDevice, st));
    d_kept = (const uint32_t*)(ws + o_kept);
  }
  uint32_t* wcnt = (uint32_t*)(ws + o_wcnt);
  int64_t* cnt = (int64_t*)(ws + o_cnt);
  int64_t* rp = (int64_t*)(ws + o_rp);  // rp[rows] = surviving edges, rp[rows + 1] = the list's error flag: one read-back
  void* scan_tmp = ws + o_scan;

  if (nw > 0) GAIB_HIP(hipMemsetAsync(bits, 0, sizeof(unsigned long long) * nw, st));
  GAIB_HIP(hipMemsetAsync(rp + rows + 1, 0, sizeof(int64_t), st));
  if (n_kept > 0) {
    ProfScope prof(ctx, "induce_mark", 12.0 * (double)n_kept);
    induce_mark_kernel<<<(unsigned)cdiv64(n_kept, 256), 256, 0, st>>>(n_kept, d_kept, nv, bits, d_rows_out, rp + rows + 1);
    GAIB_LAUNCH_CHECK();
  }
  {
    ProfScope prof(ctx, "induce_scan", 16.0 * (double)nw);
    induce_popc_kernel<<<(unsigned)cdiv64(nw + 1, 256), 256, 0, st>>>(nw, bits, wcnt);
    GAIB_LAUNCH_CHECK();
    size_t b = scan_bytes;
    GAIB_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, b, wcnt, g->induce_prefix, (int)(nw + 1), st));
  }
  {
    ProfScope prof(ctx, "induce_count");
    const unsigned grid = (unsigned)cdiv64(rows + 1, 4);
    if (relabel)
      induce_rows_kernel<false, true><<<grid, 256, 0, st>>>(rows, nv, d_kept, g->rowptr, g->colidx, bits, g->induce_prefix, cnt,
                                                            nullptr, nullptr);
    else
      induce_rows_kernel<false, false><<<grid, 256, 0, st>>>(rows, nv, d_kept, g->rowptr, g->colidx, bits, g->induce_prefix, cnt,
                                                             nullptr, nullptr);
    GAIB_LAUNCH_CHECK();
    size_t b = scan_bytes;
    GAIB_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, b, cnt, rp, (int)(rows + 1), st));
  }
  int64_t h[2] = {0, 0};  // the call's one wait
  GAIB_HIP(hipMemcpyAsync(h, rp + rows, sizeof(h), hipMemcpyDeviceToHost, st));
  GAIB_HIP(hipStreamSynchronize(st));
  if (h[1] != 0) {
    gaib_set_error("gaib_graph_induce: the kept list is not strictly ascending or holds an id >= nv (%lld)", (long long)nv);
    return GAIB_ERR_INVALID;
  }
  const int64_t ne = h[0];
  gaib_graph* r = nullptr;
  GAIB_TRY(gaib_graph_new(rows, ne, ctx->device, &r));
  hipError_t e = hipMemcpyAsync(r->rowptr, rp, sizeof(int64_t) * (rows + 1), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && rows > 0) {
    ProfScope prof(ctx, "induce_fill");
    const unsigned grid = (unsigned)cdiv64(rows, 4);
    if (relabel)
      induce_rows_kernel<true, true><<<grid, 256, 0, st>>>(rows, nv, d_kept, g->rowptr, g->colidx, bits, g->induce_prefix, nullptr,
                                                           r->rowptr, r->colidx);
    else
      induce_rows_kernel<true, false><<<grid, 256, 0, st>>>(rows, nv, d_kept, g->rowptr, g->colidx, bits, g->induce_prefix, nullptr,
                                                            r->rowptr, r->colidx);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    gaib_set_error("gaib_graph_induce: %s", hipGetErrorString(e));
    (void)gaib_graph_destroy(r);
    return GAIB_ERR_HIP;
  }
  r->rows_unsorted = g->rows_unsorted;  // (every row keeps the order of its surviving edges; ranks are monotone)
  *out = r;
  return GAIB_OK;
}

extern "C" int gaib_gather_rows_u8(gaib_ctx* ctx, int64_t n_idx, const int64_t* d_idx, int width_bytes, const uint8_t* d_in,
                                   uint8_t* d_out) {
  GAIB_CHECK(ctx && ((d_idx && d_in && d_out) || n_idx == 0), "gaib_gather_rows_u8: NULL argument");
  GAIB_CHECK(n_idx >= 0 && width_bytes >= 1, "gaib_gather_rows_u8: need n_idx >= 0 and width_bytes >= 1");
  if (n_idx == 0) return GAIB_OK;
  const int64_t total = n_idx * (int64_t)width_bytes;
  ProfScope prof(ctx, "gather_rows_u8", 2.0 * (double)total + 8.0 * (double)n_idx);
  const int64_t blocks = cdiv64(total, 256);
  gather_rows_u8_kernel<<<(unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), 256, 0, ctx->stream>>>(total, width_bytes, d_idx,
                                                                                                    d_in, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}
