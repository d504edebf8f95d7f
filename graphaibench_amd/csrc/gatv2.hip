// gatv2.hip -- the one-sweep GATv2 (include/gaib.h: gaib_gatv2_forward / gaib_gatv2_backward): argument checks, workspace and the
// launch sequences around the two sweeps of gatv2_kernels.h.
//   forward:   chunk grid (+ XCD walk), gatv2_fwd_chunk_kernel, gat_fwd_reduce_kernel (the v1 partial format: its kernel)
//   backward:  rowdot_kernel, gat_rec_kernel (records (delta, m, 1 / l)), gatv2_bwd_chunk_kernel, gat_fused_reduce_kernel (the
//              partial rows in chunk order), gatv2_agrad_strip_kernel, gatv2_agrad_final_kernel (a's gradient, two fixed levels)
// Cover: gat_fused_shape(len, heads) on whole graphs, fp32 tables below 4 GB (the sweeps address a row by a 32-bit byte offset).
// There is NO staged GATv2: outside the cover the calls return GAIB_ERR_UNSUPPORTED with nothing touched and the caller has to
// say so.  Option gat_chunk_xcd is honoured.  Deterministic, no atomics.
#include "gat_fused_seq.h"
#include "gatv2_kernels.h"

namespace {

// forward: 8 steps in flight (the v1 forward's); backward: 4 at every width (three gathers per step; 100 - 108 VGPRs, no spill,
// four waves per SIMD -- the 128-column instance needed no lower unroll)
#define GAIB_V2_FWD(GG, HH)                                                                                                    \
  gatv2_fwd_chunk_kernel<GG, HH, 8><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start,  \
                                                                   g->rowptr, g->colidx, d_h, d_a, eps, ws.out_partial,        \
                                                                   ws.ms_partial, per_xcd)
#define GAIB_V2_BWD(GG, HH)                                                                                                    \
  gatv2_bwd_chunk_kernel<GG, HH, 4><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start,  \
                                                                   g->rowptr, g->colidx, d_feat, d_grad, rec, d_a, eps,        \
                                                                   out_partial, ag_partial, per_xcd)

// what both calls refuse before they touch anything: 0 = go on
int gatv2_check(const char* who, gaib_ctx* ctx, gaib_graph* g, int len, int heads, uintptr_t align_or) {
  if (!gat_fused_shape(len, heads) || g->nc != g->nv || (uint64_t)g->nv * (uint64_t)len * 4u >= ((uint64_t)1 << 32)) {
    gaib_set_error("%s: covers len 32, 64 or 128 with 1, 2, 4, 8 or 16 heads of at least 4 columns on a whole graph over tables below "
                   "4 GB (len %d, heads %d, %lld x %lld)", who, len, heads, (long long)g->nv, (long long)g->nc);
    return GAIB_ERR_UNSUPPORTED;
  }
  GAIB_CHECK((align_or & 15) == 0, "%s: buffers must be 16-byte aligned", who);
  return GAIB_OK;
}

}  // namespace

extern "C" int gaib_gatv2_forward(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h, const float* d_a, float eps,
                                  int relu, float* d_out, float* d_row_stats) {
  const char* who = "gaib_gatv2_forward";
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_TRY(check_heads(who, len, heads));
  GAIB_TRY(gatv2_check(who, ctx, g, len, heads, (uintptr_t)d_h | (uintptr_t)d_a | (uintptr_t)d_out | (uintptr_t)d_row_stats));
  if (g->nv == 0) return GAIB_OK;
  GAIB_CHECK(d_h && d_a && d_out && d_row_stats && d_out != d_h, "%s: NULL or aliased pointer", who);
  GAIB_HIP(hipSetDevice(ctx->device));
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  FwdWs ws;
  GAIB_TRY(gat_forward_ws(ctx, g, len, heads, &ws));
  // bytes: per edge the column id and one gathered row; per chunk the partial (acc, m, l) written and read; per row its own h,
  // out and the statistics.  flops: per edge and column z, phi, the score's fma, and the accumulator's
  ProfScope ps(ctx, "gatv2_fwd", (double)g->ne * (4.0 + 4.0 * len) + (double)g->n_chunks * (4.0 * len + 8.0 * heads) * 2 +
                                     (double)g->nv * (2 * 4.0 * len + 8.0 * heads),
               7.0 * (double)g->ne * len);
  unsigned grid;
  int per_xcd;
  chunk_grid(ctx, g, true, &grid, &per_xcd);
  if (grid > 0) {
    GAIB_GAT_DISPATCH(GAIB_V2_FWD);
    GAIB_LAUNCH_CHECK();
  }
  // (rows without an edge: zeros and statistics (-1e30, 0), as in v1)
#define GAIB_V2_FR(GG)                                                                                                        \
  gat_fwd_reduce_kernel<GG><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, g->chunk_start, ws.out_partial,      \
                                                                     ws.ms_partial, relu ? 1 : 0, d_out,                     \
                                                                     reinterpret_cast<float2*>(d_row_stats))
  if (len == 32) GAIB_V2_FR(8);
  else if (len == 64) GAIB_V2_FR(16);
  else GAIB_V2_FR(32);
#undef GAIB_V2_FR
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_gatv2_backward(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat, const float* d_grad,
                                   const float* d_fwd_out, const float* d_a, const float* d_row_stats, float eps, float* d_grad_out,
                                   float* d_a_grad) {
  const char* who = "gaib_gatv2_backward";
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_TRY(check_heads(who, len, heads));
  GAIB_TRY(gatv2_check(who, ctx, g, len, heads,
                       (uintptr_t)d_feat | (uintptr_t)d_grad | (uintptr_t)d_fwd_out | (uintptr_t)d_a | (uintptr_t)d_row_stats |
                           (uintptr_t)d_grad_out | (uintptr_t)d_a_grad));
  GAIB_CHECK(d_a_grad, "%s: NULL pointer", who);
  if (g->nv == 0) return zero_alpha_grads(ctx, len, d_a_grad, nullptr);
  GAIB_CHECK(d_feat && d_grad && d_fwd_out && d_a && d_row_stats && d_grad_out, "%s: NULL pointer", who);
  GAIB_CHECK(d_grad_out != d_feat && d_grad_out != d_grad && d_grad_out != d_fwd_out, "%s: d_grad_out must not alias an input", who);
  GAIB_HIP(hipSetDevice(ctx->device));
  // the single sweep takes the in-edges of a row for the reverses of its own edges: a graph that is not structurally symmetric is
  // an error, the permutation's own (the sweep does not read it)
  GAIB_TRY(gaib_graph_ensure_rev(ctx, g));
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  unsigned grid;
  int per_xcd;
  chunk_grid(ctx, g, true, &grid, &per_xcd);
  const int nstrips = grid == 0 ? 0 : (int)(grid < 4096 ? cdiv64(grid, 4) : 1024);
  // workspace: records [nv][heads] x 16 B | rowdot [nv][heads] | partial rows [n_chunks][len] | a-gradient partials [grid][len] |
  // their strips [nstrips][len]
  const size_t n_v = up4((size_t)g->nv * heads), n_op = up4((size_t)g->n_chunks * len);
  const size_t n_ag = (size_t)grid * len, n_st = (size_t)nstrips * len;
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (5 * n_v + n_op + n_ag + n_st)));
  f4* rec = reinterpret_cast<f4*>(ctx->ws);
  float* rowdot = (float*)ctx->ws + 4 * n_v;
  float* out_partial = rowdot + n_v;
  float* ag_partial = out_partial + n_op;
  float* ag_strip = ag_partial + n_ag;
  // bytes: per edge the column id, two gathered rows and the 12 bytes of a record per head; per chunk the partial row written and
  // read; per row h, grad and the forward output read, grad_out written and 20 bytes per head of statistics and record; per
  // workgroup its a-gradient partial written and read.  flops: per edge and column the score (5), two dots (4), the three
  // accumulators (6)
  ProfScope ps(ctx, "gatv2_bwd", (double)g->ne * (4.0 + 2 * 4.0 * len + 12.0 * heads) + (double)g->n_chunks * 4.0 * len * 2 +
                                     (double)g->nv * (4 * 4.0 * len + 20.0 * heads) + (double)grid * 4.0 * len * 2,
               15.0 * (double)g->ne * len);
  GAIB_TRY((gat_bwd_prologue<float, false>(ctx, g->nv, len, heads, len, heads, d_grad, d_fwd_out, d_row_stats, rowdot, rec)));
  if (grid > 0) {
    GAIB_GAT_DISPATCH(GAIB_V2_BWD);
    GAIB_LAUNCH_CHECK();
    gatv2_agrad_strip_kernel<<<nstrips, 256, 0, ctx->stream>>>((int64_t)grid, len, ag_partial, cdiv64(grid, nstrips), ag_strip);
    GAIB_LAUNCH_CHECK();
  }
  gatv2_agrad_final_kernel<<<(unsigned)cdiv64(len, 4), 256, 0, ctx->stream>>>(nstrips, len, ag_strip, d_a_grad);
  GAIB_LAUNCH_CHECK();
  // the rows' partial sums in chunk order (H = 0: the kernel's row / column sums of v1 have no part here, nothing of them is read
  // or written)
#define GAIB_V2_RD(GG)                                                                                                              \
  gat_fused_reduce_kernel<GG><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, 0, g->chunk_start, out_partial, nullptr, d_grad_out, \
                                                                       nullptr, nullptr)
  if (len == 32) GAIB_V2_RD(8);
  else if (len == 64) GAIB_V2_RD(16);
  else GAIB_V2_RD(32);
#undef GAIB_V2_RD
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}
