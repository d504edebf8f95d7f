// gat_drop.hip -- the one-sweep GAT forward and backward under attention dropout (option "gat_fused_drop" of the layer library).
// The kernels are the DROP variants of the two sweeps of gat_kernels.h on fp32 tables: the mask of (edge e, head k) is the one
// gaib_dropout draws for element e * heads + k of an [ne][heads] array under the same seed, formed inside the sweep
// (gat_drop_bits) -- no [ne][heads] array exists on this path either.
//   forward:  out_i = act(sum_e p_e w_e h_c), w = mask . scale; the softmax and so d_row_stats do not see the mask
//   backward: dp_e = w_e <grad_i, h_c>, dp_r = w_r <grad_c, h_i>, out_i += p_r w_r grad_c with r = rev(e); rowdot_v = <grad_v, out_v>
//             is still sum_e p_e dp_e of row v with the dropped output, so the records and everything after the sweep are those of
//             gaib_gat_backward_fused (row-statistics form)
// With rate 0 and scale 1 every w is 1.0f and a product by it changes no bit: the results are the undropped calls'.
// The reverse edge's mask needs rev(e): a graph without a reverse-edge permutation is refused by forward and backward alike.
// With option gat_fused_wide = 1 a multi-head row wider than 128 columns goes to the slab loop of gat_wide.hip, where every slab
// reaches its heads' masks through a window of the [ne][heads] index (gaib_gat_*_fused_drop_win).
#include "gat_kernels.h"

static int gat_drop_refuse(const char* who, int len, int heads) {
  gaib_set_error("%s: not applicable to this shape / graph (len %d, heads %d)", who, len, heads);
  return GAIB_ERR_UNSUPPORTED;
}

extern "C" int gaib_gat_forward_fused_drop(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h, const float* d_alpha_l,
                                           const float* d_alpha_r, float epsilon, int relu, float drop_rate, float scale, uint64_t seed,
                                           float* d_out, float* d_row_stats) {
  const char* who = "gaib_gat_forward_fused_drop";
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_CHECK(len > 0 && heads >= 1 && len % heads == 0, "%s: heads (%d) must divide len (%d)", who, heads, len);
  GAIB_CHECK(drop_rate >= 0.f && drop_rate < 1.f, "%s: rate must be in [0,1)", who);
  if (g->nv == 0 || g->nc != g->nv) return gat_drop_refuse(who, len, heads);  // (no rows: as gaib_gat_forward_fused; no _rect form)
  GAIB_CHECK(d_h && d_alpha_l && d_alpha_r && d_out && d_row_stats && d_out != d_h, "%s: NULL or aliased pointer", who);
  GAIB_HIP(hipSetDevice(ctx->device));
  // option gat_fused_wide: a multi-head row wider than 128 columns as S column slabs, each with its window of the mask (gat_wide.hip)
  if (ctx->gat_fused_wide == 1 && !gat_fused_shape(len, heads)) {
    int w = 0;
    const int S = gaib_gat_fused_slabs(len, heads, &w);
    if (S >= 2)
      return gaib_gat_forward_fused_drop_wide(ctx, g, len, heads, w, S, d_h, d_alpha_l, d_alpha_r, epsilon, relu, drop_rate, scale, seed,
                                              d_out, d_row_stats);
  }
  int rc = GAIB_OK;
  const uintptr_t align_or = (uintptr_t)d_h | (uintptr_t)d_out | (uintptr_t)d_row_stats | (uintptr_t)d_alpha_l | (uintptr_t)d_alpha_r;
  if (!gat_fused_applies(ctx, g, len, heads, ctx->gat_fused_fwd, align_or, &rc)) return gat_drop_refuse(who, len, heads);
  GAIB_TRY(gaib_graph_ensure_rev(ctx, g));  // (not read here: forward and backward must decide alike)
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  const size_t n_op = up4((size_t)g->n_chunks * len), n_ms = up4((size_t)g->n_chunks * heads * 2);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (n_op + n_ms)));
  float* out_partial = (float*)ctx->ws;
  float2* ms_partial = reinterpret_cast<float2*>(out_partial + n_op);
  // profile key and byte formula of the undropped call: the mask moves no byte
  ProfScope ps(ctx, "gat_fwd_fused", (double)g->ne * (4.0 + 4.0 * len) + (double)g->n_chunks * (4.0 * len + 8.0 * heads) * 2 + (double)g->nv * (4.0 * len + 8.0 * heads),
               4.0 * (double)g->ne * len);
  unsigned grid = (unsigned)cdiv64(g->n_chunks, 4);
  int per_xcd = 0;
  if (ctx->gat_chunk_xcd == 1 && grid >= 64) {
    per_xcd = (int)cdiv64(grid, 8);
    grid = (unsigned)per_xcd * 8u;
  }
#define GAIB_FF(GG, HH)                                                                                                       \
  gat_fwd_fused_chunk_kernel<GG, HH, 8, float, true><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, \
                                                                            g->chunk_start, g->rowptr, g->colidx, len, d_h,   \
                                                                            d_alpha_l, d_alpha_r, epsilon, out_partial,       \
                                                                            ms_partial, -1, (uint32_t)g->nv, per_xcd,         \
                                                                            drop_rate, scale, seed)
  GAIB_GAT_DISPATCH(GAIB_FF);
#undef GAIB_FF
  GAIB_LAUNCH_CHECK();
#define GAIB_FR(GG)                                                                                                        \
  gat_fwd_reduce_kernel<GG><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, g->chunk_start, out_partial, ms_partial, \
                                                                     relu ? 1 : 0, d_out, reinterpret_cast<float2*>(d_row_stats))
  if (len == 32) GAIB_FR(8);
  else if (len == 64) GAIB_FR(16);
  else GAIB_FR(32);
#undef GAIB_FR
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_gat_backward_fused_drop(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat, const float* d_grad,
                                            const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                                            const float* d_row_stats, float epsilon, float drop_rate, float scale, uint64_t seed,
                                            float* d_grad_out, float* d_alpha_lgrad, float* d_alpha_rgrad) {
  const char* who = "gaib_gat_backward_fused_drop";
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_CHECK(len > 0 && heads >= 1 && len % heads == 0, "%s: heads (%d) must divide len (%d)", who, heads, len);
  GAIB_CHECK(drop_rate >= 0.f && drop_rate < 1.f, "%s: rate must be in [0,1)", who);
  if (g->nv == 0) {  // no rows: the alpha gradients of this graph are zero, nothing else is written (as gaib_gat_backward_fused)
    GAIB_HIP(hipSetDevice(ctx->device));
    if (d_alpha_lgrad) GAIB_HIP(hipMemsetAsync(d_alpha_lgrad, 0, sizeof(float) * len, ctx->stream));
    if (d_alpha_rgrad) GAIB_HIP(hipMemsetAsync(d_alpha_rgrad, 0, sizeof(float) * len, ctx->stream));
    return GAIB_OK;
  }
  GAIB_CHECK(d_row_stats, "%s: d_row_stats is NULL (the dropped sweep has no attention-array form)", who);
  GAIB_CHECK(d_feat && d_grad && d_fwd_out && d_alpha_l && d_alpha_r && d_grad_out && d_alpha_lgrad && d_alpha_rgrad,
             "%s: NULL pointer", who);
  GAIB_CHECK(d_grad_out != d_feat && d_grad_out != d_grad, "%s: d_grad_out must not alias an input", who);
  if (g->nc != g->nv) return gat_drop_refuse(who, len, heads);
  GAIB_HIP(hipSetDevice(ctx->device));
  if (ctx->gat_fused_wide == 1 && !gat_fused_shape(len, heads)) {  // (see the forward)
    int w = 0;
    const int S = gaib_gat_fused_slabs(len, heads, &w);
    if (S >= 2)
      return gaib_gat_backward_fused_drop_wide(ctx, g, len, heads, w, S, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r, d_row_stats,
                                               epsilon, drop_rate, scale, seed, d_grad_out, d_alpha_lgrad, d_alpha_rgrad);
  }
  int rc0 = GAIB_OK;
  const uintptr_t align_or = (uintptr_t)d_feat | (uintptr_t)d_grad | (uintptr_t)d_row_stats | (uintptr_t)d_grad_out;
  if (!gat_fused_applies(ctx, g, len, heads, ctx->gat_fused_bwd, align_or, &rc0)) return gat_drop_refuse(who, len, heads);
  GAIB_TRY(gaib_graph_ensure_rev(ctx, g));  // the reverse edge's mask is the one of element rev(e) * heads + k
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  const int nblocks = (int)(g->nv < 2048 ? cdiv64(g->nv, 8) : 1024);
  const int64_t rows_per_block = cdiv64(g->nv, nblocks);
  auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  const size_t n_v = up4((size_t)g->nv * heads);
  const size_t n_op = up4((size_t)g->n_chunks * len), n_rc = up4((size_t)g->n_chunks * 2 * heads);
  // options gat_bwd_pk and gat_interleave are ignored: the chunk kernel over the three tables runs
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (7 * n_v + n_op + n_rc + (size_t)nblocks * 2 * len)));
  f4* rec = reinterpret_cast<f4*>(ctx->ws);  // [nv][H] 16-byte records (first: alignment)
  float* rowdot = (float*)ctx->ws + 4 * n_v;
  float* rs = rowdot + n_v;
  float* cs = rs + n_v;
  float* out_partial = cs + n_v;
  float* rc_partial = out_partial + n_op;
  float* partial = rc_partial + n_rc;
  ProfScope ps(ctx, "gat_bwd_fused", (double)g->ne * (4.0 + 2 * 4.0 * len + 12.0 * heads) + (double)g->n_chunks * (4.0 * len + 8.0 * heads) * 2 + (double)g->nv * 3 * 4.0 * len,
               8.0 * (double)g->ne * len);
  rowdot_kernel<<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, d_grad, d_fwd_out, rowdot);
  GAIB_LAUNCH_CHECK();
  const int64_t nrec = g->nv * (int64_t)heads;
  gat_rec_kernel<<<(unsigned)cdiv64(nrec, 256), 256, 0, ctx->stream>>>(nrec, rowdot, reinterpret_cast<const float2*>(d_row_stats), rec);
  GAIB_LAUNCH_CHECK();
  unsigned grid = (unsigned)cdiv64(g->n_chunks, 4);
  int per_xcd = 0;
  if (ctx->gat_chunk_xcd == 1 && grid >= 64) {
    per_xcd = (int)cdiv64(grid, 8);
    grid = (unsigned)per_xcd * 8u;
  }
#define GAIB_FB_U(GG, HH, UU)                                                                                              \
  gat_bwd_fused_chunk_kernel<GG, HH, UU, true, float, true><<<grid, 256, 0, ctx->stream>>>(                                \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, g->rev, len, d_feat, d_grad,        \
      nullptr, reinterpret_cast<const float2*>(d_row_stats), rowdot, d_alpha_l, d_alpha_r, epsilon, out_partial,           \
      rc_partial, rec, -1, 0u, len, heads, per_xcd, drop_rate, scale, seed)
  // (8 edges in flight per group: option gat_fused_unroll, the 64-wide form only, as in the undropped call)
#define GAIB_FB(GG, HH)                                                     \
  do {                                                                      \
    if (GG == 16 && ctx->gat_fused_unroll == 8) GAIB_FB_U(16, HH, 8);        \
    else GAIB_FB_U(GG, HH, 4);                                              \
  } while (0)
  GAIB_GAT_DISPATCH(GAIB_FB);
#undef GAIB_FB
#undef GAIB_FB_U
  GAIB_LAUNCH_CHECK();
#define GAIB_FRD(GG)                                                                                                   \
  gat_fused_reduce_kernel<GG><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, g->chunk_start, out_partial, \
                                                                       rc_partial, d_grad_out, rs, cs)
  if (len == 32) GAIB_FRD(8);
  else if (len == 64) GAIB_FRD(16);
  else GAIB_FRD(32);
#undef GAIB_FRD
  GAIB_LAUNCH_CHECK();
  alpha_partial_kernel<<<nblocks, 256, sizeof(float) * 512, ctx->stream>>>(g->nv, len, heads, d_feat, rs, cs, rows_per_block,
                                                                         partial);
  GAIB_LAUNCH_CHECK();
  alpha_final_kernel<<<(unsigned)cdiv64(2 * (int64_t)len, 4), 256, 0, ctx->stream>>>(nblocks, len, partial, d_alpha_lgrad,
                                                                                    d_alpha_rgrad);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}
