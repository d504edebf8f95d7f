// gat_wide_slabs.h -- the host sequences of the one-sweep GAT on column slabs (option "gat_fused_wide"), on the element type E of
// the gathered tables: E = float (gat_wide.hip) or uint16_t = raw bf16 bits (gat_wide_bf16.hip).  One text for both: a slab of
// the forward, a slab of the backward, the loops over the slabs and the window sequence at a narrow shape.  Only the tables
// (h; feat and grad) have the type E; records, statistics, alpha vectors, partial sums and every output are fp32 in both.
// Each translation unit that includes this instantiates the WIDE / WIN kernels of gat_kernels.h on its own E.
#pragma once
#include "gat_kernels.h"

namespace {

// gat_rec_kernel with the row statistics read from a window of Hs heads in [nv][stats_ld] records: rec stays [nv][Hs]
__global__ void gat_rec_wide_kernel(int64_t n, int Hs, int stats_ld, const float* rowdot, const float2* stats, f4* rec) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    const int64_t v = t / Hs;
    const float2 st = stats[v * stats_ld + (t - v * Hs)];
    rec[t] = f4{rowdot[t], st.x, st.y, 0.f};
  }
}

size_t up4(size_t n) { return (n + 3) & ~(size_t)3; }

// attention dropout on a slab: rate, scale and seed of the call, and the slab's window into the [ne][mask_heads] mask array
struct DropWin {
  float rate, scale;
  uint64_t seed;
  int mask_heads, mask_head0;
};

int wide_refuse(const char* who, int len, int heads) {
  gaib_set_error("%s: not applicable to this shape / graph (len %d, heads %d)", who, len, heads);
  return GAIB_ERR_UNSUPPORTED;
}

// a table's part in the 16-byte alignment test of the fp32 buffers: an fp32 table as it is; a bf16 table must be 8-byte aligned
// (a lane's four columns are one 8-byte load), reported as a miss of the 16
uintptr_t table_align(const float* p) { return (uintptr_t)p; }
uintptr_t table_align(const uint16_t* p) { return ((uintptr_t)p & 7) ? 15 : 0; }

// the narrow calls' conditions beside the shape: a square graph with edges, aligned buffers, the option not 0
bool wide_applies(const gaib_graph* g, int knob, uintptr_t align_or) {
  return g->nc == g->nv && g->ne > 0 && (align_or & 15) == 0 && knob != 0;
}

void chunk_grid(const gaib_ctx* ctx, const gaib_graph* g, unsigned* grid, int* per_xcd) {
  *grid = (unsigned)cdiv64(g->n_chunks, 4);
  *per_xcd = 0;
  if (ctx->gat_chunk_xcd == 1 && *grid >= 64) {
    *per_xcd = (int)cdiv64(*grid, 8);
    *grid = (unsigned)*per_xcd * 8u;
  }
}

}  // namespace

// One slab of the forward: len / heads are the SLAB's (w, Hs) -- what GAIB_GAT_DISPATCH reads --, ld / stats_ld the strides of
// the caller's tables and of d_row_stats (float2 records); every pointer is already at the slab's first column / head.
// dw: NULL, or the slab's attention dropout (the DROP sweep with the head window).
template <typename E>
static int gat_forward_slab(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int ld, int stats_ld, const E* d_h,
                            const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float* d_out, float2* stats,
                            float* out_partial, float2* ms_partial, const DropWin* dw = nullptr) {
  unsigned grid;
  int per_xcd;
  chunk_grid(ctx, g, &grid, &per_xcd);
#define GAIB_FFD(GG, HH)                                                                                                      \
  gat_fwd_fused_chunk_kernel<GG, HH, 8, E, true, true><<<grid, 256, 0, ctx->stream>>>(                                        \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, len, d_h, d_alpha_l, d_alpha_r, epsilon, \
      out_partial, ms_partial, -1, (uint32_t)g->nv, per_xcd, dw->rate, dw->scale, dw->seed, ld, dw->mask_heads, dw->mask_head0)
#define GAIB_FF(GG, HH)                                                                                                       \
  gat_fwd_fused_chunk_kernel<GG, HH, 8, E, false, true><<<grid, 256, 0, ctx->stream>>>(                                       \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, len, d_h, d_alpha_l, d_alpha_r, epsilon, \
      out_partial, ms_partial, -1, (uint32_t)g->nv, per_xcd, 0.0f, 1.0f, 0, ld)
  if (dw) GAIB_GAT_DISPATCH(GAIB_FFD);
  else GAIB_GAT_DISPATCH(GAIB_FF);
#undef GAIB_FF
#undef GAIB_FFD
  GAIB_LAUNCH_CHECK();
#define GAIB_FR(GG)                                                                                                     \
  gat_fwd_reduce_kernel<GG, true><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, g->chunk_start, out_partial, \
                                                                           ms_partial, relu ? 1 : 0, d_out, stats, ld, stats_ld)
  if (len == 32) GAIB_FR(8);
  else if (len == 64) GAIB_FR(16);
  else GAIB_FR(32);
#undef GAIB_FR
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// drop: NULL, or rate / scale / seed of a dropped call (the loop sets every slab's window); the graph's reverse-edge permutation
// is then built here, as in the narrow dropped call: forward and backward must decide alike
template <typename E>
static int gat_forward_wide(const char* who, gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const E* d_h,
                            const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float* d_out,
                            float* d_row_stats, const DropWin* drop) {
  const uintptr_t align_or = table_align(d_h) | (uintptr_t)d_out | (uintptr_t)d_row_stats | (uintptr_t)d_alpha_l | (uintptr_t)d_alpha_r;
  if (!wide_applies(g, ctx->gat_fused_fwd, align_or)) return wide_refuse(who, len, heads);
  const int Hs = heads / S;
  if (drop) GAIB_TRY(gaib_graph_ensure_rev(ctx, g));
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  const size_t n_op = up4((size_t)g->n_chunks * w), n_ms = up4((size_t)g->n_chunks * Hs * 2);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (n_op + n_ms)));
  float* out_partial = (float*)ctx->ws;
  float2* ms_partial = reinterpret_cast<float2*>(out_partial + n_op);
  // the narrow call's formula at (w, Hs), S times: the column ids and the chunk headers are read once per slab
  // (the fp32 formula on bf16 tables too: the achieved rate is a work rate in dense bytes)
  ProfScope ps(ctx, "gat_fwd_fused",
               S * ((double)g->ne * (4.0 + 4.0 * w) + (double)g->n_chunks * (4.0 * w + 8.0 * Hs) * 2 + (double)g->nv * (4.0 * w + 8.0 * Hs)),
               4.0 * (double)g->ne * len);
  for (int s = 0; s < S; ++s) {
    const int c0 = s * w;
    DropWin dw = {0.f, 1.f, 0, heads, s * Hs};
    if (drop) dw.rate = drop->rate, dw.scale = drop->scale, dw.seed = drop->seed;
    GAIB_TRY(gat_forward_slab(ctx, g, w, Hs, len, heads, d_h + c0, d_alpha_l + c0, d_alpha_r + c0, epsilon, relu, d_out + c0,
                              reinterpret_cast<float2*>(d_row_stats) + s * Hs, out_partial, ms_partial, drop ? &dw : nullptr));
  }
  return GAIB_OK;
}

// One slab of the backward (row-statistics form); names as in gat_forward_slab (dw: the graph's reverse-edge permutation exists)
template <typename E>
static int gat_backward_slab(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int ld, int stats_ld, const E* d_feat,
                             const E* d_grad, const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                             const float2* stats, float epsilon, float* d_grad_out, float* d_alpha_lgrad, float* d_alpha_rgrad,
                             f4* rec, float* rowdot, float* rs, float* cs, float* out_partial, float* rc_partial, float* partial,
                             int nblocks, int64_t rows_per_block, const DropWin* dw = nullptr) {
  rowdot_kernel<E, true><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, d_grad, d_fwd_out, rowdot, ld);
  GAIB_LAUNCH_CHECK();
  const int64_t nrec = g->nv * (int64_t)heads;
  gat_rec_wide_kernel<<<(unsigned)cdiv64(nrec, 256), 256, 0, ctx->stream>>>(nrec, heads, stats_ld, rowdot, stats, rec);
  GAIB_LAUNCH_CHECK();
  unsigned grid;
  int per_xcd;
  chunk_grid(ctx, g, &grid, &per_xcd);
  // the chunk kernel takes its row strides as they are (ld, rec_ld: added for the interleaved table); the records are the slab's own
#define GAIB_FB_U(GG, HH, UU)                                                                                              \
  gat_bwd_fused_chunk_kernel<GG, HH, UU, true, E><<<grid, 256, 0, ctx->stream>>>(                                          \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, nullptr, len, d_feat, d_grad, nullptr, \
      nullptr, nullptr, d_alpha_l, d_alpha_r, epsilon, out_partial, rc_partial, rec, -1, 0u, ld, heads, per_xcd)
#define GAIB_FBD_U(GG, HH, UU)                                                                                             \
  gat_bwd_fused_chunk_kernel<GG, HH, UU, true, E, true, true><<<grid, 256, 0, ctx->stream>>>(                              \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, g->rev, len, d_feat, d_grad, nullptr, \
      nullptr, nullptr, d_alpha_l, d_alpha_r, epsilon, out_partial, rc_partial, rec, -1, 0u, ld, heads, per_xcd, dw->rate, \
      dw->scale, dw->seed, dw->mask_heads, dw->mask_head0)
  // (8 edges in flight per group: option gat_fused_unroll, the 64-wide form only, as in the narrow call)
#define GAIB_FB(GG, HH)                                               \
  do {                                                                \
    if (GG == 16 && ctx->gat_fused_unroll == 8) GAIB_FB_U(16, HH, 8); \
    else GAIB_FB_U(GG, HH, 4);                                        \
  } while (0)
#define GAIB_FBD(GG, HH)                                               \
  do {                                                                 \
    if (GG == 16 && ctx->gat_fused_unroll == 8) GAIB_FBD_U(16, HH, 8); \
    else GAIB_FBD_U(GG, HH, 4);                                        \
  } while (0)
  if (dw) GAIB_GAT_DISPATCH(GAIB_FBD);
  else GAIB_GAT_DISPATCH(GAIB_FB);
#undef GAIB_FB
#undef GAIB_FBD
#undef GAIB_FB_U
#undef GAIB_FBD_U
  GAIB_LAUNCH_CHECK();
#define GAIB_FRD(GG)                                                                                                       \
  gat_fused_reduce_kernel<GG, true><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, g->chunk_start, out_partial, \
                                                                             rc_partial, d_grad_out, rs, cs, ld)
  if (len == 32) GAIB_FRD(8);
  else if (len == 64) GAIB_FRD(16);
  else GAIB_FRD(32);
#undef GAIB_FRD
  GAIB_LAUNCH_CHECK();
  alpha_partial_kernel<E, true><<<nblocks, 256, sizeof(float) * 512, ctx->stream>>>(g->nv, len, heads, d_feat, rs, cs,
                                                                                  rows_per_block, partial, ld);
  GAIB_LAUNCH_CHECK();
  alpha_final_kernel<<<(unsigned)cdiv64(2 * (int64_t)len, 4), 256, 0, ctx->stream>>>(nblocks, len, partial, d_alpha_lgrad,
                                                                                    d_alpha_rgrad);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// the backward's workspace at the width (w, Hs) of one slab, or of the whole row in the window sequence
struct BwdWs {
  f4* rec;  // [nv][Hs] 16-byte records (first: alignment)
  float *rowdot, *rs, *cs, *out_partial, *rc_partial, *partial;
  int nblocks;
  int64_t rows_per_block;
};
static int gat_backward_ws(gaib_ctx* ctx, const gaib_graph* g, int w, int Hs, BwdWs* ws) {
  ws->nblocks = (int)(g->nv < 2048 ? cdiv64(g->nv, 8) : 1024);
  ws->rows_per_block = cdiv64(g->nv, ws->nblocks);
  const size_t n_v = up4((size_t)g->nv * Hs);
  const size_t n_op = up4((size_t)g->n_chunks * w), n_rc = up4((size_t)g->n_chunks * 2 * Hs);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (7 * n_v + n_op + n_rc + (size_t)ws->nblocks * 2 * w)));
  ws->rec = reinterpret_cast<f4*>(ctx->ws);
  ws->rowdot = (float*)ctx->ws + 4 * n_v;
  ws->rs = ws->rowdot + n_v;
  ws->cs = ws->rs + n_v;
  ws->out_partial = ws->cs + n_v;
  ws->rc_partial = ws->out_partial + n_op;
  ws->partial = ws->rc_partial + n_rc;
  return GAIB_OK;
}

template <typename E>
static int gat_backward_wide(const char* who, gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const E* d_feat,
                             const E* d_grad, const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                             const float* d_row_stats, float epsilon, float* d_grad_out, float* d_alpha_lgrad,
                             float* d_alpha_rgrad, const DropWin* drop) {
  const uintptr_t align_or = table_align(d_feat) | table_align(d_grad) | (uintptr_t)d_row_stats | (uintptr_t)d_grad_out;
  if (!wide_applies(g, ctx->gat_fused_bwd, align_or)) return wide_refuse(who, len, heads);
  const int Hs = heads / S;
  if (drop) GAIB_TRY(gaib_graph_ensure_rev(ctx, g));  // the reverse edge's mask is the one of element rev(e) * heads + head
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  BwdWs ws;
  GAIB_TRY(gat_backward_ws(ctx, g, w, Hs, &ws));
  ProfScope ps(ctx, "gat_bwd_fused",
               S * ((double)g->ne * (4.0 + 2 * 4.0 * w + 12.0 * Hs) + (double)g->n_chunks * (4.0 * w + 8.0 * Hs) * 2 + (double)g->nv * 3 * 4.0 * w),
               8.0 * (double)g->ne * len);
  for (int s = 0; s < S; ++s) {
    const int c0 = s * w;
    DropWin dw = {0.f, 1.f, 0, heads, s * Hs};
    if (drop) dw.rate = drop->rate, dw.scale = drop->scale, dw.seed = drop->seed;
    GAIB_TRY(gat_backward_slab(ctx, g, w, Hs, len, heads, d_feat + c0, d_grad + c0, d_fwd_out + c0, d_alpha_l + c0, d_alpha_r + c0,
                               reinterpret_cast<const float2*>(d_row_stats) + s * Hs, epsilon, d_grad_out + c0, d_alpha_lgrad + c0,
                               d_alpha_rgrad + c0, ws.rec, ws.rowdot, ws.rs, ws.cs, ws.out_partial, ws.rc_partial, ws.partial,
                               ws.nblocks, ws.rows_per_block, drop ? &dw : nullptr));
  }
  return GAIB_OK;
}

// ---- the window sequence at a narrow shape, contiguous tables: one slab with ld = len, stats_ld = heads ---------------------------
// (gaib_gat_*_fused_drop_win on fp32 tables; with the window (heads, 0) on bf16 tables it is gaib_gat_*_fused_drop_bf16)
template <typename E>
static int gat_forward_win(const char* who, gaib_ctx* ctx, gaib_graph* g, int len, int heads, const E* d_h, const float* d_alpha_l,
                           const float* d_alpha_r, float epsilon, int relu, float drop_rate, float scale, uint64_t seed,
                           int mask_heads, int mask_head0, float* d_out, float* d_row_stats) {
  int rc = GAIB_OK;
  const uintptr_t align_or = table_align(d_h) | (uintptr_t)d_out | (uintptr_t)d_row_stats | (uintptr_t)d_alpha_l | (uintptr_t)d_alpha_r;
  if (!gat_fused_applies(ctx, g, len, heads, ctx->gat_fused_fwd, align_or, &rc)) return wide_refuse(who, len, heads);
  GAIB_TRY(gaib_graph_ensure_rev(ctx, g));  // (not read here: forward and backward must decide alike)
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  const size_t n_op = up4((size_t)g->n_chunks * len), n_ms = up4((size_t)g->n_chunks * heads * 2);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (n_op + n_ms)));
  float* out_partial = (float*)ctx->ws;
  float2* ms_partial = reinterpret_cast<float2*>(out_partial + n_op);
  ProfScope ps(ctx, "gat_fwd_fused",
               (double)g->ne * (4.0 + 4.0 * len) + (double)g->n_chunks * (4.0 * len + 8.0 * heads) * 2 + (double)g->nv * (4.0 * len + 8.0 * heads),
               4.0 * (double)g->ne * len);
  const DropWin dw = {drop_rate, scale, seed, mask_heads, mask_head0};
  return gat_forward_slab(ctx, g, len, heads, len, heads, d_h, d_alpha_l, d_alpha_r, epsilon, relu, d_out,
                          reinterpret_cast<float2*>(d_row_stats), out_partial, ms_partial, &dw);
}

template <typename E>
static int gat_backward_win(const char* who, gaib_ctx* ctx, gaib_graph* g, int len, int heads, const E* d_feat, const E* d_grad,
                            const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r, const float* d_row_stats,
                            float epsilon, float drop_rate, float scale, uint64_t seed, int mask_heads, int mask_head0,
                            float* d_grad_out, float* d_alpha_lgrad, float* d_alpha_rgrad) {
  int rc0 = GAIB_OK;
  const uintptr_t align_or = table_align(d_feat) | table_align(d_grad) | (uintptr_t)d_row_stats | (uintptr_t)d_grad_out;
  if (!gat_fused_applies(ctx, g, len, heads, ctx->gat_fused_bwd, align_or, &rc0)) return wide_refuse(who, len, heads);
  GAIB_TRY(gaib_graph_ensure_rev(ctx, g));
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  BwdWs ws;
  GAIB_TRY(gat_backward_ws(ctx, g, len, heads, &ws));
  ProfScope ps(ctx, "gat_bwd_fused",
               (double)g->ne * (4.0 + 2 * 4.0 * len + 12.0 * heads) + (double)g->n_chunks * (4.0 * len + 8.0 * heads) * 2 + (double)g->nv * 3 * 4.0 * len,
               8.0 * (double)g->ne * len);
  const DropWin dw = {drop_rate, scale, seed, mask_heads, mask_head0};
  return gat_backward_slab(ctx, g, len, heads, len, heads, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r,
                           reinterpret_cast<const float2*>(d_row_stats), epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad, ws.rec,
                           ws.rowdot, ws.rs, ws.cs, ws.out_partial, ws.rc_partial, ws.partial, ws.nblocks, ws.rows_per_block, &dw);
}
