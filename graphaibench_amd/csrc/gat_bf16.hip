// gat_bf16.hip -- the one-sweep GAT forward and backward over bf16 tables (option "gat_bf16" of the layer library).
// The kernels are those of gat_kernels.h with the element type E = uint16_t: every read of h and grad -- own rows and gathered
// rows in the sweeps, grad in rowdot, h in the alpha gradients -- takes raw bf16 bits and widens them exactly (a shift / a mask),
// on the consume side of the batch's sched_barrier; everything behind the widening is the fp32 kernel's text.  So the results
// are the bits of gaib_gat_forward_fused / gaib_gat_backward_fused (row-statistics form) on the widened tables, under the
// same options.  A gathered row is 2 len bytes instead of 4 len: at 8 heads x 8 the backward sweep touches three 128-byte
// lines per edge (h, grad, records) instead of five.
// With option gat_fused_wide = 1 a multi-head row wider than 128 columns goes to the slab loop on bf16 tables (gat_wide_bf16.hip),
// where the calls under attention dropout (gaib_gat_*_fused_drop_bf16) live too.
#include "gat_kernels.h"

static int gat_bf16_refuse(const char* who, int len, int heads) {
  gaib_set_error("%s: not applicable to this shape / graph (len %d, heads %d)", who, len, heads);
  return GAIB_ERR_UNSUPPORTED;
}

extern "C" int gaib_gat_forward_fused_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_h_bf16,
                                           const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu,
                                           float* d_out, float* d_row_stats) {
  const char* who = "gaib_gat_forward_fused_bf16";
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_CHECK(len > 0 && heads >= 1 && len % heads == 0, "%s: heads (%d) must divide len (%d)", who, heads, len);
  if (g->nv == 0) return gat_bf16_refuse(who, len, heads);  // (as gaib_gat_forward_fused on a square graph)
  GAIB_CHECK(d_h_bf16 && d_alpha_l && d_alpha_r && d_out && d_row_stats && (const void*)d_out != (const void*)d_h_bf16,
             "%s: NULL or aliased pointer", who);
  GAIB_HIP(hipSetDevice(ctx->device));
  // option gat_fused_wide: a multi-head row wider than 128 columns as S column slabs of the bf16 table (gat_wide_bf16.hip)
  if (ctx->gat_fused_wide == 1 && !gat_fused_shape(len, heads)) {
    int w = 0;
    const int S = gaib_gat_fused_slabs(len, heads, &w);
    if (S >= 2)
      return gaib_gat_forward_fused_bf16_wide(ctx, g, len, heads, w, S, d_h_bf16, d_alpha_l, d_alpha_r, epsilon, relu, d_out, d_row_stats);
  }
  int rc = GAIB_OK;
  // the bf16 table: 8-byte aligned (a lane's four columns are one 8-byte load); the fp32 buffers 16 bytes as in the fp32 call
  const uintptr_t align_or = ((uintptr_t)d_h_bf16 & 7 ? 15 : 0) | (uintptr_t)d_out | (uintptr_t)d_row_stats |
                             (uintptr_t)d_alpha_l | (uintptr_t)d_alpha_r;
  if (!gat_fused_applies(ctx, g, len, heads, ctx->gat_fused_fwd, align_or, &rc)) return gat_bf16_refuse(who, len, heads);
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  const size_t n_op = up4((size_t)g->n_chunks * len), n_ms = up4((size_t)g->n_chunks * heads * 2);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (n_op + n_ms)));
  float* out_partial = (float*)ctx->ws;
  float2* ms_partial = reinterpret_cast<float2*>(out_partial + n_op);
  // profile key and byte formula of the fp32 call: the achieved rate is a work rate in dense (fp32) bytes
  ProfScope ps(ctx, "gat_fwd_fused", (double)g->ne * (4.0 + 4.0 * len) + (double)g->n_chunks * (4.0 * len + 8.0 * heads) * 2 + (double)g->nv * (4.0 * len + 8.0 * heads),
               4.0 * (double)g->ne * len);
  unsigned grid = (unsigned)cdiv64(g->n_chunks, 4);
  int per_xcd = 0;
  if (ctx->gat_chunk_xcd == 1 && grid >= 64) {
    per_xcd = (int)cdiv64(grid, 8);
    grid = (unsigned)per_xcd * 8u;
  }
#define GAIB_FF(GG, HH)                                                                                                        \
  gat_fwd_fused_chunk_kernel<GG, HH, 8, uint16_t><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase,    \
                                                                                 g->chunk_start, g->rowptr, g->colidx, len,   \
                                                                                 d_h_bf16, d_alpha_l, d_alpha_r, epsilon,     \
                                                                                 out_partial, ms_partial, -1, (uint32_t)g->nv, \
                                                                                 per_xcd)
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

extern "C" int gaib_gat_backward_fused_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_feat_bf16,
                                            const uint16_t* d_grad_bf16, const float* d_fwd_out, const float* d_alpha_l,
                                            const float* d_alpha_r, const float* d_row_stats, float epsilon, float* d_grad_out,
                                            float* d_alpha_lgrad, float* d_alpha_rgrad) {
  const char* who = "gaib_gat_backward_fused_bf16";
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_CHECK(len > 0 && heads >= 1 && len % heads == 0, "%s: heads (%d) must divide len (%d)", who, heads, len);
  if (g->nv == 0) {  // no rows: the alpha gradients of this graph are zero, nothing else is written (as gaib_gat_backward_fused)
    GAIB_HIP(hipSetDevice(ctx->device));
    if (d_alpha_lgrad) GAIB_HIP(hipMemsetAsync(d_alpha_lgrad, 0, sizeof(float) * len, ctx->stream));
    if (d_alpha_rgrad) GAIB_HIP(hipMemsetAsync(d_alpha_rgrad, 0, sizeof(float) * len, ctx->stream));
    return GAIB_OK;
  }
  GAIB_CHECK(d_row_stats, "%s: d_row_stats is NULL (the bf16 sweep has no attention-array form)", who);
  GAIB_CHECK(d_feat_bf16 && d_grad_bf16 && d_fwd_out && d_alpha_l && d_alpha_r && d_grad_out && d_alpha_lgrad && d_alpha_rgrad,
             "%s: NULL pointer", who);
  GAIB_CHECK((const void*)d_grad_out != (const void*)d_feat_bf16 && (const void*)d_grad_out != (const void*)d_grad_bf16,
             "%s: d_grad_out must not alias an input", who);
  GAIB_HIP(hipSetDevice(ctx->device));
  if (ctx->gat_fused_wide == 1 && !gat_fused_shape(len, heads)) {  // (see the forward)
    int w = 0;
    const int S = gaib_gat_fused_slabs(len, heads, &w);
    if (S >= 2)
      return gaib_gat_backward_fused_bf16_wide(ctx, g, len, heads, w, S, d_feat_bf16, d_grad_bf16, d_fwd_out, d_alpha_l, d_alpha_r,
                                               d_row_stats, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad);
  }
  int rc0 = GAIB_OK;
  const uintptr_t align_or = ((((uintptr_t)d_feat_bf16 | (uintptr_t)d_grad_bf16) & 7) ? 15 : 0) | (uintptr_t)d_row_stats |
                             (uintptr_t)d_grad_out;
  if (!gat_fused_applies(ctx, g, len, heads, ctx->gat_fused_bwd, align_or, &rc0)) return gat_bf16_refuse(who, len, heads);
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  const int nblocks = (int)(g->nv < 2048 ? cdiv64(g->nv, 8) : 1024);
  const int64_t rows_per_block = cdiv64(g->nv, nblocks);
  auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  const size_t n_v = up4((size_t)g->nv * heads);
  const size_t n_op = up4((size_t)g->n_chunks * len), n_rc = up4((size_t)g->n_chunks * 2 * heads);
  // the packed-math sweep (option gat_bwd_pk = 1) over rows of len dwords (h_k low half, g_k high half) + the fp32 records:
  // 4 len + 16 heads bytes per vertex, the 32-bit byte-offset condition taken on that size.  Option gat_interleave is ignored:
  // the bf16 rows are gathered from their own tables, which changes no bits in fp32 either.
  const int ldt = len + 4 * heads;  // dwords of a packed row
  const bool pk = ctx->gat_bwd_pk == 1 && (len / 4) / heads <= 16 && (uint64_t)g->nv * (uint64_t)ldt * 4u < ((uint64_t)1 << 32);
  const size_t n_t = pk ? up4((size_t)g->nv * ldt) + 64 : 0;  // (+ 64 floats: the table starts on a 256-B boundary)
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (7 * n_v + n_op + n_rc + (size_t)nblocks * 2 * len + n_t)));
  f4* rec = reinterpret_cast<f4*>(ctx->ws);  // [nv][H] 16-byte records (first: alignment)
  float* rowdot = (float*)ctx->ws + 4 * n_v;
  float* rs = rowdot + n_v;
  float* cs = rs + n_v;
  float* out_partial = cs + n_v;
  float* rc_partial = out_partial + n_op;
  float* partial = rc_partial + n_rc;
  uint16_t* T = reinterpret_cast<uint16_t*>(((uintptr_t)(partial + (size_t)nblocks * 2 * len) + 255) & ~(uintptr_t)255);
  ProfScope ps(ctx, "gat_bwd_fused", (double)g->ne * (4.0 + 2 * 4.0 * len + 12.0 * heads) + (double)g->n_chunks * (4.0 * len + 8.0 * heads) * 2 + (double)g->nv * 3 * 4.0 * len,
               8.0 * (double)g->ne * len);
  rowdot_kernel<<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, d_grad_bf16, d_fwd_out, rowdot);
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
  if (pk) {
    const int64_t tot4 = g->nv * (int64_t)(ldt / 4);
    gat_pairs_bf16_kernel<<<(unsigned)std::min<int64_t>(cdiv64(tot4, 256), (int64_t)ctx->num_cus * 16), 256, 0, ctx->stream>>>(
        g->nv, len / 4, heads, reinterpret_cast<const u32x2*>(d_feat_bf16), reinterpret_cast<const u32x2*>(d_grad_bf16), rec,
        reinterpret_cast<u32x4*>(T));
    GAIB_LAUNCH_CHECK();
#define GAIB_FBP(GG, HH)                                                                                                      \
  launch_bwd_pk<GG, HH, uint16_t>(grid, ctx->stream, g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr,    \
                                  g->colidx, len, T, d_alpha_l, d_alpha_r, epsilon, out_partial, rc_partial, per_xcd)
    GAIB_GAT_DISPATCH(GAIB_FBP);
#undef GAIB_FBP
    GAIB_LAUNCH_CHECK();
  } else {
#define GAIB_FB_U(GG, HH, UU)                                                                                              \
  gat_bwd_fused_chunk_kernel<GG, HH, UU, true, uint16_t><<<grid, 256, 0, ctx->stream>>>(                                   \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, nullptr, len, d_feat_bf16,          \
      d_grad_bf16, nullptr, reinterpret_cast<const float2*>(d_row_stats), rowdot, d_alpha_l, d_alpha_r, epsilon,           \
      out_partial, rc_partial, rec, -1, 0u, len, heads, per_xcd)
  // (8 edges in flight per group: option gat_fused_unroll, the 64-wide form only, as in fp32)
#define GAIB_FB(GG, HH)                                                     \
  do {                                                                      \
    if (GG == 16 && ctx->gat_fused_unroll == 8) GAIB_FB_U(16, HH, 8);        \
    else GAIB_FB_U(GG, HH, 4);                                              \
  } while (0)
    GAIB_GAT_DISPATCH(GAIB_FB);
#undef GAIB_FB
#undef GAIB_FB_U
    GAIB_LAUNCH_CHECK();
  }
#define GAIB_FRD(GG)                                                                                                   \
  gat_fused_reduce_kernel<GG><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, g->chunk_start, out_partial, \
                                                                       rc_partial, d_grad_out, rs, cs)
  if (len == 32) GAIB_FRD(8);
  else if (len == 64) GAIB_FRD(16);
  else GAIB_FRD(32);
#undef GAIB_FRD
  GAIB_LAUNCH_CHECK();
  alpha_partial_kernel<<<nblocks, 256, sizeof(float) * 512, ctx->stream>>>(g->nv, len, heads, d_feat_bf16, rs, cs, rows_per_block,
                                                                         partial);
  GAIB_LAUNCH_CHECK();
  alpha_final_kernel<<<(unsigned)cdiv64(2 * (int64_t)len, 4), 256, 0, ctx->stream>>>(nblocks, len, partial, d_alpha_lgrad,
                                                                                    d_alpha_rgrad);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}
