// gat_wide.hip -- the one-sweep GAT forward and backward on multi-head rows wider than 128 columns (option "gat_fused_wide").
// Heads are independent in everything the two sweeps compute, so a row of len = S w columns with heads = S Hs heads is S
// independent problems of w columns and Hs heads, each in a column window [s w, (s + 1) w) of the same tables: a shape the
// G = 8 / 16 / 32 lane layouts of gat_kernels.h already run, with a row STRIDE (len) that differs from the row WIDTH (w).  The
// kernels here are the WIDE instantiations of those kernels -- the same instructions on strided rows -- and a call is a loop
// over the slabs on the context's stream, each slab the narrow call's own sequence at (w, Hs):
//   forward:  chunk sweep, gat_fwd_reduce_kernel                      -> columns of d_out, heads of d_row_stats [nv][heads][2]
//   backward: rowdot, records, chunk sweep, gat_fused_reduce_kernel,
//             alpha_partial_kernel, alpha_final_kernel                -> columns of d_grad_out and of the two alpha gradients
// The chunk list, the order of a chunk's steps, the chunk-order reductions and the block partition of the alpha reductions
// follow from the graph and nv alone, so every slab's outputs are BIT-IDENTICAL to the narrow call at (len = w, heads = Hs) on
// contiguous copies of its column windows.  Deterministic, no atomics.
// What a slab keeps to itself lives in the workspace at the slab's own width and is reused by the next slab (same stream): the
// per-chunk partials (n_chunks w floats, not n_chunks len), rowdot, the records and rs / cs [nv][Hs], the alpha partials.
// Only the caller's arrays are strided: the tables [nv][len] and d_row_stats [nv][heads][2].
// Options: gat_chunk_xcd is honoured, gat_fused_unroll = 8 where w == 64; gat_bwd_pk and gat_interleave are ignored (the chunk
// kernel over the three separate tables runs, as in the _drop calls).
// Under ATTENTION DROPOUT (gaib_gat_*_fused_drop with the option on) the slab sequence is the same with the DROP sweeps, and the
// mask of (edge e, head k of slab s) is the full row's: element e heads + s Hs + k of the virtual [ne][heads] mask array, which a
// slab reaches through a head WINDOW (mask_heads = heads, mask_head0 = s Hs; gat_drop_bits<.., WIN>).  The window sequence at a
// narrow shape on contiguous tables is an entry point of its own (gaib_gat_*_fused_drop_win): the unit a wide dropped call is made of.
// The sequences themselves are templates on the tables' element type (gat_wide_slabs.h), shared with gat_wide_bf16.hip.
#include "gat_wide_slabs.h"

// the shape rule (include/gaib.h): pure, no context, no device
extern "C" int gaib_gat_fused_slabs(int len, int heads, int* width) {
  int w = 0, S = 0;
  if (len > 0 && heads >= 1) {
    if (gat_fused_shape(len, heads)) {
      w = len;
      S = 1;
    } else {
      const int widths[] = {128, 64, 32};  // widest first: the fewest re-reads of column ids and chunk headers
      for (int cand : widths) {
        if (len % cand != 0 || len / cand < 2 || heads % (len / cand) != 0) continue;
        if (!gat_fused_shape(cand, heads / (len / cand))) continue;
        w = cand;
        S = len / cand;
        break;
      }
    }
  }
  if (width) *width = w;
  return S;
}

int gaib_gat_forward_fused_wide(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const float* d_h,
                                const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float* d_out,
                                float* d_row_stats) {
  return gat_forward_wide<float>("gaib_gat_forward_fused", ctx, g, len, heads, w, S, d_h, d_alpha_l, d_alpha_r, epsilon, relu, d_out,
                                 d_row_stats, nullptr);
}

int gaib_gat_forward_fused_drop_wide(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const float* d_h,
                                     const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float drop_rate,
                                     float scale, uint64_t seed, float* d_out, float* d_row_stats) {
  const DropWin drop = {drop_rate, scale, seed, heads, 0};
  return gat_forward_wide<float>("gaib_gat_forward_fused_drop", ctx, g, len, heads, w, S, d_h, d_alpha_l, d_alpha_r, epsilon, relu, d_out,
                                 d_row_stats, &drop);
}

int gaib_gat_backward_fused_wide(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const float* d_feat,
                                 const float* d_grad, const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                                 const float* d_row_stats, float epsilon, float* d_grad_out, float* d_alpha_lgrad,
                                 float* d_alpha_rgrad) {
  return gat_backward_wide<float>("gaib_gat_backward_fused", ctx, g, len, heads, w, S, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r,
                                  d_row_stats, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad, nullptr);
}

int gaib_gat_backward_fused_drop_wide(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const float* d_feat,
                                      const float* d_grad, const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                                      const float* d_row_stats, float epsilon, float drop_rate, float scale, uint64_t seed,
                                      float* d_grad_out, float* d_alpha_lgrad, float* d_alpha_rgrad) {
  const DropWin drop = {drop_rate, scale, seed, heads, 0};
  return gat_backward_wide<float>("gaib_gat_backward_fused_drop", ctx, g, len, heads, w, S, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r,
                                  d_row_stats, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad, &drop);
}

// ---- the window sequence at a narrow shape, contiguous tables (include/gaib.h): one slab with ld = len, stats_ld = heads ----------
extern "C" int gaib_gat_forward_fused_drop_win(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h,
                                               const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu,
                                               float drop_rate, float scale, uint64_t seed, int mask_heads, int mask_head0,
                                               float* d_out, float* d_row_stats) {
  const char* who = "gaib_gat_forward_fused_drop_win";
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_CHECK(len > 0 && heads >= 1 && len % heads == 0, "%s: heads (%d) must divide len (%d)", who, heads, len);
  GAIB_CHECK(drop_rate >= 0.f && drop_rate < 1.f, "%s: rate must be in [0,1)", who);
  GAIB_CHECK(mask_head0 >= 0 && (int64_t)mask_head0 + heads <= (int64_t)mask_heads,
             "%s: heads [%d, %d + %d) are no window of %d mask heads", who, mask_head0, mask_head0, heads, mask_heads);
  if (g->nv == 0 || g->nc != g->nv) return wide_refuse(who, len, heads);
  GAIB_CHECK(d_h && d_alpha_l && d_alpha_r && d_out && d_row_stats && d_out != d_h, "%s: NULL or aliased pointer", who);
  GAIB_HIP(hipSetDevice(ctx->device));
  return gat_forward_win<float>(who, ctx, g, len, heads, d_h, d_alpha_l, d_alpha_r, epsilon, relu, drop_rate, scale, seed, mask_heads,
                                mask_head0, d_out, d_row_stats);
}

extern "C" int gaib_gat_backward_fused_drop_win(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat,
                                                const float* d_grad, const float* d_fwd_out, const float* d_alpha_l,
                                                const float* d_alpha_r, const float* d_row_stats, float epsilon, float drop_rate,
                                                float scale, uint64_t seed, int mask_heads, int mask_head0, float* d_grad_out,
                                                float* d_alpha_lgrad, float* d_alpha_rgrad) {
  const char* who = "gaib_gat_backward_fused_drop_win";
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_CHECK(len > 0 && heads >= 1 && len % heads == 0, "%s: heads (%d) must divide len (%d)", who, heads, len);
  GAIB_CHECK(drop_rate >= 0.f && drop_rate < 1.f, "%s: rate must be in [0,1)", who);
  GAIB_CHECK(mask_head0 >= 0 && (int64_t)mask_head0 + heads <= (int64_t)mask_heads,
             "%s: heads [%d, %d + %d) are no window of %d mask heads", who, mask_head0, mask_head0, heads, mask_heads);
  if (g->nv == 0) {  // no rows: zero alpha gradients, nothing else is written (as gaib_gat_backward_fused_drop)
    GAIB_HIP(hipSetDevice(ctx->device));
    if (d_alpha_lgrad) GAIB_HIP(hipMemsetAsync(d_alpha_lgrad, 0, sizeof(float) * len, ctx->stream));
    if (d_alpha_rgrad) GAIB_HIP(hipMemsetAsync(d_alpha_rgrad, 0, sizeof(float) * len, ctx->stream));
    return GAIB_OK;
  }
  GAIB_CHECK(d_row_stats, "%s: d_row_stats is NULL (the dropped sweep has no attention-array form)", who);
  GAIB_CHECK(d_feat && d_grad && d_fwd_out && d_alpha_l && d_alpha_r && d_grad_out && d_alpha_lgrad && d_alpha_rgrad,
             "%s: NULL pointer", who);
  GAIB_CHECK(d_grad_out != d_feat && d_grad_out != d_grad, "%s: d_grad_out must not alias an input", who);
  if (g->nc != g->nv) return wide_refuse(who, len, heads);
  GAIB_HIP(hipSetDevice(ctx->device));
  return gat_backward_win<float>(who, ctx, g, len, heads, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r, d_row_stats, epsilon,
                                 drop_rate, scale, seed, mask_heads, mask_head0, d_grad_out, d_alpha_lgrad, d_alpha_rgrad);
}
