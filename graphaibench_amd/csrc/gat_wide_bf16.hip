// gat_wide_bf16.hip -- the one-sweep GAT over bf16 TABLES where the sweep is a DROP or a WIDE form: under attention dropout
// (gaib_gat_*_fused_drop_bf16, option "gat_fused_drop" of the layer library) and on multi-head rows wider than 128 columns
// (option "gat_fused_wide": the _bf16 calls and the _drop_bf16 calls), and both at once.
// The host sequences are those of gat_wide_slabs.h on E = uint16_t, the kernels the WIDE / WIN instantiations of gat_kernels.h on
// raw bf16 bits: a lane's four columns of a row are one 8-byte load, widened exactly (a shift / a mask) on the consume side of the
// batch's sched_barrier, and everything behind the widening is the fp32 kernel's text.  So every output has the bits of the
// corresponding fp32 call on the tables widened to fp32, under the same options and the same (rate, scale, seed):
//   _drop_bf16 at a narrow shape  = _drop         (the window sequence with ld = len and the window (heads, 0): DESIGN 3.3.3)
//   _bf16      at a wide shape    = gaib_gat_*_fused, wide
//   _drop_bf16 at a wide shape    = _drop, wide
// Slab s gathers from column s w of the bf16 tables with the row stride len: 2 s w bytes, a multiple of 64 for every slab width,
// so the 8-byte loads stay aligned.  gat_chunk_xcd is honoured, gat_fused_unroll = 8 where the (slab) width is 64; gat_bwd_pk
// and gat_interleave are ignored.  Deterministic, no atomics.  Profile: the fp32 calls' keys and byte formulas (a work rate in
// dense bytes).
#include "gat_wide_slabs.h"

// ---- the undropped _bf16 calls on S >= 2 column slabs: called by gat_bf16.hip after its argument checks ---------------------------
int gaib_gat_forward_fused_bf16_wide(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const uint16_t* d_h_bf16,
                                     const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float* d_out,
                                     float* d_row_stats) {
  return gat_forward_wide<uint16_t>("gaib_gat_forward_fused_bf16", ctx, g, len, heads, w, S, d_h_bf16, d_alpha_l, d_alpha_r, epsilon,
                                    relu, d_out, d_row_stats, nullptr);
}

int gaib_gat_backward_fused_bf16_wide(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const uint16_t* d_feat_bf16,
                                      const uint16_t* d_grad_bf16, const float* d_fwd_out, const float* d_alpha_l,
                                      const float* d_alpha_r, const float* d_row_stats, float epsilon, float* d_grad_out,
                                      float* d_alpha_lgrad, float* d_alpha_rgrad) {
  return gat_backward_wide<uint16_t>("gaib_gat_backward_fused_bf16", ctx, g, len, heads, w, S, d_feat_bf16, d_grad_bf16, d_fwd_out,
                                     d_alpha_l, d_alpha_r, d_row_stats, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad, nullptr);
}

// ---- attention dropout on bf16 tables (include/gaib.h): the argument checks of gaib_gat_*_fused_drop ------------------------------
extern "C" int gaib_gat_forward_fused_drop_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_h_bf16,
                                                const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu,
                                                float drop_rate, float scale, uint64_t seed, float* d_out, float* d_row_stats) {
  const char* who = "gaib_gat_forward_fused_drop_bf16";
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_CHECK(len > 0 && heads >= 1 && len % heads == 0, "%s: heads (%d) must divide len (%d)", who, heads, len);
  GAIB_CHECK(drop_rate >= 0.f && drop_rate < 1.f, "%s: rate must be in [0,1)", who);
  if (g->nv == 0 || g->nc != g->nv) return wide_refuse(who, len, heads);  // (no rows: as gaib_gat_forward_fused; no _rect form)
  GAIB_CHECK(d_h_bf16 && d_alpha_l && d_alpha_r && d_out && d_row_stats && (const void*)d_out != (const void*)d_h_bf16,
             "%s: NULL or aliased pointer", who);
  GAIB_HIP(hipSetDevice(ctx->device));
  if (ctx->gat_fused_wide == 1 && !gat_fused_shape(len, heads)) {
    int w = 0;
    const int S = gaib_gat_fused_slabs(len, heads, &w);
    if (S >= 2) {
      const DropWin drop = {drop_rate, scale, seed, heads, 0};
      return gat_forward_wide<uint16_t>(who, ctx, g, len, heads, w, S, d_h_bf16, d_alpha_l, d_alpha_r, epsilon, relu, d_out,
                                        d_row_stats, &drop);
    }
  }
  return gat_forward_win<uint16_t>(who, ctx, g, len, heads, d_h_bf16, d_alpha_l, d_alpha_r, epsilon, relu, drop_rate, scale, seed,
                                   heads, 0, d_out, d_row_stats);
}

extern "C" int gaib_gat_backward_fused_drop_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_feat_bf16,
                                                 const uint16_t* d_grad_bf16, const float* d_fwd_out, const float* d_alpha_l,
                                                 const float* d_alpha_r, const float* d_row_stats, float epsilon, float drop_rate,
                                                 float scale, uint64_t seed, float* d_grad_out, float* d_alpha_lgrad,
                                                 float* d_alpha_rgrad) {
  const char* who = "gaib_gat_backward_fused_drop_bf16";
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_CHECK(len > 0 && heads >= 1 && len % heads == 0, "%s: heads (%d) must divide len (%d)", who, heads, len);
  GAIB_CHECK(drop_rate >= 0.f && drop_rate < 1.f, "%s: rate must be in [0,1)", who);
  if (g->nv == 0) {  // no rows: the alpha gradients of this graph are zero, nothing else is written (as gaib_gat_backward_fused_drop)
    GAIB_HIP(hipSetDevice(ctx->device));
    if (d_alpha_lgrad) GAIB_HIP(hipMemsetAsync(d_alpha_lgrad, 0, sizeof(float) * len, ctx->stream));
    if (d_alpha_rgrad) GAIB_HIP(hipMemsetAsync(d_alpha_rgrad, 0, sizeof(float) * len, ctx->stream));
    return GAIB_OK;
  }
  GAIB_CHECK(d_row_stats, "%s: d_row_stats is NULL (the dropped sweep has no attention-array form)", who);
  GAIB_CHECK(d_feat_bf16 && d_grad_bf16 && d_fwd_out && d_alpha_l && d_alpha_r && d_grad_out && d_alpha_lgrad && d_alpha_rgrad,
             "%s: NULL pointer", who);
  GAIB_CHECK((const void*)d_grad_out != (const void*)d_feat_bf16 && (const void*)d_grad_out != (const void*)d_grad_bf16,
             "%s: d_grad_out must not alias an input", who);
  if (g->nc != g->nv) return wide_refuse(who, len, heads);
  GAIB_HIP(hipSetDevice(ctx->device));
  if (ctx->gat_fused_wide == 1 && !gat_fused_shape(len, heads)) {
    int w = 0;
    const int S = gaib_gat_fused_slabs(len, heads, &w);
    if (S >= 2) {
      const DropWin drop = {drop_rate, scale, seed, heads, 0};
      return gat_backward_wide<uint16_t>(who, ctx, g, len, heads, w, S, d_feat_bf16, d_grad_bf16, d_fwd_out, d_alpha_l, d_alpha_r,
                                         d_row_stats, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad, &drop);
    }
  }
  return gat_backward_win<uint16_t>(who, ctx, g, len, heads, d_feat_bf16, d_grad_bf16, d_fwd_out, d_alpha_l, d_alpha_r, d_row_stats,
                                    epsilon, drop_rate, scale, seed, heads, 0, d_grad_out, d_alpha_lgrad, d_alpha_rgrad);
}
