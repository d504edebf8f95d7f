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

// the narrow calls' conditions beside the shape: a square graph with edges, 16-byte aligned buffers, the option not 0
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

// One slab of the forward: len / heads are the SLAB's (w, Hs) -- what GAIB_GAT_DISPATCH reads --, ld / stats_ld the strides of
// the caller's tables and of d_row_stats (float2 records); every pointer is already at the slab's first column / head.
// dw: NULL, or the slab's attention dropout (the DROP sweep with the head window).
static int gat_forward_slab(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int ld, int stats_ld, const float* d_h,
                            const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float* d_out, float2* stats,
                            float* out_partial, float2* ms_partial, const DropWin* dw = nullptr) {
  unsigned grid;
  int per_xcd;
  chunk_grid(ctx, g, &grid, &per_xcd);
#define GAIB_FFD(GG, HH)                                                                                                      \
  gat_fwd_fused_chunk_kernel<GG, HH, 8, float, true, true><<<grid, 256, 0, ctx->stream>>>(                                    \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, len, d_h, d_alpha_l, d_alpha_r, epsilon, \
      out_partial, ms_partial, -1, (uint32_t)g->nv, per_xcd, dw->rate, dw->scale, dw->seed, ld, dw->mask_heads, dw->mask_head0)
#define GAIB_FF(GG, HH)                                                                                                       \
  gat_fwd_fused_chunk_kernel<GG, HH, 8, float, false, true><<<grid, 256, 0, ctx->stream>>>(                                   \
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
static int gat_forward_wide(const char* who, gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const float* d_h,
                            const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float* d_out,
                            float* d_row_stats, const DropWin* drop) {
  const uintptr_t align_or = (uintptr_t)d_h | (uintptr_t)d_out | (uintptr_t)d_row_stats | (uintptr_t)d_alpha_l | (uintptr_t)d_alpha_r;
  if (!wide_applies(g, ctx->gat_fused_fwd, align_or)) return wide_refuse(who, len, heads);
  const int Hs = heads / S;
  if (drop) GAIB_TRY(gaib_graph_ensure_rev(ctx, g));
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  const size_t n_op = up4((size_t)g->n_chunks * w), n_ms = up4((size_t)g->n_chunks * Hs * 2);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (n_op + n_ms)));
  float* out_partial = (float*)ctx->ws;
  float2* ms_partial = reinterpret_cast<float2*>(out_partial + n_op);
  // the narrow call's formula at (w, Hs), S times: the column ids and the chunk headers are read once per slab
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

int gaib_gat_forward_fused_wide(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const float* d_h,
                                const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float* d_out,
                                float* d_row_stats) {
  return gat_forward_wide("gaib_gat_forward_fused", ctx, g, len, heads, w, S, d_h, d_alpha_l, d_alpha_r, epsilon, relu, d_out,
                          d_row_stats, nullptr);
}

int gaib_gat_forward_fused_drop_wide(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const float* d_h,
                                     const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu, float drop_rate,
                                     float scale, uint64_t seed, float* d_out, float* d_row_stats) {
  const DropWin drop = {drop_rate, scale, seed, heads, 0};
  return gat_forward_wide("gaib_gat_forward_fused_drop", ctx, g, len, heads, w, S, d_h, d_alpha_l, d_alpha_r, epsilon, relu, d_out,
                          d_row_stats, &drop);
}

// One slab of the backward (row-statistics form); names as in gat_forward_slab (dw: the graph's reverse-edge permutation exists)
static int gat_backward_slab(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int ld, int stats_ld, const float* d_feat,
                             const float* d_grad, const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                             const float2* stats, float epsilon, float* d_grad_out, float* d_alpha_lgrad, float* d_alpha_rgrad,
                             f4* rec, float* rowdot, float* rs, float* cs, float* out_partial, float* rc_partial, float* partial,
                             int nblocks, int64_t rows_per_block, const DropWin* dw = nullptr) {
  rowdot_kernel<float, true><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, d_grad, d_fwd_out, rowdot, ld);
  GAIB_LAUNCH_CHECK();
  const int64_t nrec = g->nv * (int64_t)heads;
  gat_rec_wide_kernel<<<(unsigned)cdiv64(nrec, 256), 256, 0, ctx->stream>>>(nrec, heads, stats_ld, rowdot, stats, rec);
  GAIB_LAUNCH_CHECK();
  unsigned grid;
  int per_xcd;
  chunk_grid(ctx, g, &grid, &per_xcd);
  // the chunk kernel takes its row strides as they are (ld, rec_ld: added for the interleaved table); the records are the slab's own
#define GAIB_FB_U(GG, HH, UU)                                                                                              \
  gat_bwd_fused_chunk_kernel<GG, HH, UU, true, float><<<grid, 256, 0, ctx->stream>>>(                                      \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, nullptr, len, d_feat, d_grad, nullptr, \
      nullptr, nullptr, d_alpha_l, d_alpha_r, epsilon, out_partial, rc_partial, rec, -1, 0u, ld, heads, per_xcd)
#define GAIB_FBD_U(GG, HH, UU)                                                                                             \
  gat_bwd_fused_chunk_kernel<GG, HH, UU, true, float, true, true><<<grid, 256, 0, ctx->stream>>>(                          \
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
  alpha_partial_kernel<float, true><<<nblocks, 256, sizeof(float) * 512, ctx->stream>>>(g->nv, len, heads, d_feat, rs, cs,
                                                                                      rows_per_block, partial, ld);
  GAIB_LAUNCH_CHECK();
  alpha_final_kernel<<<(unsigned)cdiv64(2 * (int64_t)len, 4), 256, 0, ctx->stream>>>(nblocks, len, partial, d_alpha_lgrad,
                                                                                    d_alpha_rgrad);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

static int gat_backward_wide(const char* who, gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const float* d_feat,
                             const float* d_grad, const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                             const float* d_row_stats, float epsilon, float* d_grad_out, float* d_alpha_lgrad,
                             float* d_alpha_rgrad, const DropWin* drop) {
  const uintptr_t align_or = (uintptr_t)d_feat | (uintptr_t)d_grad | (uintptr_t)d_row_stats | (uintptr_t)d_grad_out;
  if (!wide_applies(g, ctx->gat_fused_bwd, align_or)) return wide_refuse(who, len, heads);
  const int Hs = heads / S;
  if (drop) GAIB_TRY(gaib_graph_ensure_rev(ctx, g));  // the reverse edge's mask is the one of element rev(e) * heads + head
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  const int nblocks = (int)(g->nv < 2048 ? cdiv64(g->nv, 8) : 1024);
  const int64_t rows_per_block = cdiv64(g->nv, nblocks);
  const size_t n_v = up4((size_t)g->nv * Hs);
  const size_t n_op = up4((size_t)g->n_chunks * w), n_rc = up4((size_t)g->n_chunks * 2 * Hs);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (7 * n_v + n_op + n_rc + (size_t)nblocks * 2 * w)));
  f4* rec = reinterpret_cast<f4*>(ctx->ws);  // [nv][Hs] 16-byte records (first: alignment)
  float* rowdot = (float*)ctx->ws + 4 * n_v;
  float* rs = rowdot + n_v;
  float* cs = rs + n_v;
  float* out_partial = cs + n_v;
  float* rc_partial = out_partial + n_op;
  float* partial = rc_partial + n_rc;
  ProfScope ps(ctx, "gat_bwd_fused",
               S * ((double)g->ne * (4.0 + 2 * 4.0 * w + 12.0 * Hs) + (double)g->n_chunks * (4.0 * w + 8.0 * Hs) * 2 + (double)g->nv * 3 * 4.0 * w),
               8.0 * (double)g->ne * len);
  for (int s = 0; s < S; ++s) {
    const int c0 = s * w;
    DropWin dw = {0.f, 1.f, 0, heads, s * Hs};
    if (drop) dw.rate = drop->rate, dw.scale = drop->scale, dw.seed = drop->seed;
    GAIB_TRY(gat_backward_slab(ctx, g, w, Hs, len, heads, d_feat + c0, d_grad + c0, d_fwd_out + c0, d_alpha_l + c0, d_alpha_r + c0,
                               reinterpret_cast<const float2*>(d_row_stats) + s * Hs, epsilon, d_grad_out + c0, d_alpha_lgrad + c0,
                               d_alpha_rgrad + c0, rec, rowdot, rs, cs, out_partial, rc_partial, partial, nblocks, rows_per_block,
                               drop ? &dw : nullptr));
  }
  return GAIB_OK;
}

int gaib_gat_backward_fused_wide(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const float* d_feat,
                                 const float* d_grad, const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                                 const float* d_row_stats, float epsilon, float* d_grad_out, float* d_alpha_lgrad,
                                 float* d_alpha_rgrad) {
  return gat_backward_wide("gaib_gat_backward_fused", ctx, g, len, heads, w, S, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r,
                           d_row_stats, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad, nullptr);
}

int gaib_gat_backward_fused_drop_wide(gaib_ctx* ctx, gaib_graph* g, int len, int heads, int w, int S, const float* d_feat,
                                      const float* d_grad, const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                                      const float* d_row_stats, float epsilon, float drop_rate, float scale, uint64_t seed,
                                      float* d_grad_out, float* d_alpha_lgrad, float* d_alpha_rgrad) {
  const DropWin drop = {drop_rate, scale, seed, heads, 0};
  return gat_backward_wide("gaib_gat_backward_fused_drop", ctx, g, len, heads, w, S, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r,
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
  int rc = GAIB_OK;
  const uintptr_t align_or = (uintptr_t)d_h | (uintptr_t)d_out | (uintptr_t)d_row_stats | (uintptr_t)d_alpha_l | (uintptr_t)d_alpha_r;
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
  int rc0 = GAIB_OK;
  const uintptr_t align_or = (uintptr_t)d_feat | (uintptr_t)d_grad | (uintptr_t)d_row_stats | (uintptr_t)d_grad_out;
  if (!gat_fused_applies(ctx, g, len, heads, ctx->gat_fused_bwd, align_or, &rc0)) return wide_refuse(who, len, heads);
  GAIB_TRY(gaib_graph_ensure_rev(ctx, g));
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  const int nblocks = (int)(g->nv < 2048 ? cdiv64(g->nv, 8) : 1024);
  const int64_t rows_per_block = cdiv64(g->nv, nblocks);
  const size_t n_v = up4((size_t)g->nv * heads);
  const size_t n_op = up4((size_t)g->n_chunks * len), n_rc = up4((size_t)g->n_chunks * 2 * heads);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (7 * n_v + n_op + n_rc + (size_t)nblocks * 2 * len)));
  f4* rec = reinterpret_cast<f4*>(ctx->ws);  // [nv][heads] 16-byte records (first: alignment)
  float* rowdot = (float*)ctx->ws + 4 * n_v;
  float* rs = rowdot + n_v;
  float* cs = rs + n_v;
  float* out_partial = cs + n_v;
  float* rc_partial = out_partial + n_op;
  float* partial = rc_partial + n_rc;
  ProfScope ps(ctx, "gat_bwd_fused",
               (double)g->ne * (4.0 + 2 * 4.0 * len + 12.0 * heads) + (double)g->n_chunks * (4.0 * len + 8.0 * heads) * 2 + (double)g->nv * 3 * 4.0 * len,
               8.0 * (double)g->ne * len);
  const DropWin dw = {drop_rate, scale, seed, mask_heads, mask_head0};
  return gat_backward_slab(ctx, g, len, heads, len, heads, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r,
                           reinterpret_cast<const float2*>(d_row_stats), epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad, rec, rowdot,
                           rs, cs, out_partial, rc_partial, partial, nblocks, rows_per_block, &dw);
}
