// gat_narrow.hip -- the one-sweep GAT and GATv2 at rows of 16 and 8 columns (option "gat_fused_narrow"): the reference's default
// hidden width (DEFAULT_SIZE_HID = 16) and the one below it.  The shape rule is gat_narrow_shape (gat_kernels.h): len 16 with 1, 2 or
// 4 heads, len 8 with 1 or 2 -- heads * 4 <= len continued downwards.  The public calls (plain, _drop, _bf16, _drop_bf16; GAT from
// the row statistics, GATv2) reach the launches below through gat_narrow_forward_seq / gat_narrow_backward_seq (gat_fused_seq.h)
// and the `narrow` route of gatv2_seq.h, which check the call, lay out the narrow call's workspace at (len, heads) and run its
// rowdot, record, alpha- and a-gradient kernels around the sweep.  Every kernel at G = 4, 2 is instantiated here and nowhere else.
//
// Lanes (ChunkLanes<4>, ChunkLanes<2>): a row is G = 4 or 2 lanes of four columns, so a wave works on NG = 16 or 32 edges per step
// and a 64-edge chunk is 4 or 2 steps.  Lane (DPP row r, position p) holds the column id of edge p*4 + r, fetched once per chunk;
// group (r, q) at step t works on edge (4t + q)*4 + r (G = 4, q = (lane >> 2) & 3) or (8t + q)*4 + r (G = 2, q = (lane >> 1) & 7):
// row-shares with constant lane numbers and a select on q, no LDS and no ds_bpermute.  The edges of step t are t*NG .. t*NG + NG - 1
// as at every other width.  A head owns LH = G / H lanes in {4, 2, 1}: its sums are DPP inside the quad (LH = 1: the identity).
//
// ONE BATCH PER CHUNK: U = G.  All 4 (2) steps' gathers -- 16 (32) rows per step, 64 rows of 64, 32 or 16 bytes per wave -- are
// issued ahead of the sched_barrier before the first is consumed; at 4 steps there is nothing to gain from a shorter batch and a
// batch of raw rows costs 4 to 16 registers.  The GATv2 forward's online softmax then takes ONE maximum and ONE rescale per chunk.
// So gat_fused_unroll, gat_bwd_pk and gat_interleave have no part at these shapes; gat_chunk_xcd is honoured.
//
// The NG groups meet in the kernels' fixed-order loop (o = G .. 32: 4 or 5 stages); the partials keep their formats ([slot][len],
// [slot][H]), so gat_fwd_reduce_kernel, gat_fused_reduce_kernel and the strip kernels of a's gradient are the other widths' at
// G = 4, 2.  Attention dropout: gat_drop_bits<G, H, ..> leaves 4 or 2 mask bits per lane and chunk (bit t = step t), element
// e * heads + k, gaib_dropout's draw; the reverse edges' word reads rev at the lane's own steps.  bf16 tables: a lane's four
// columns are one 8-byte load (rows of 32 or 16 bytes), widened exactly on the consume side (Row4<E>), so every output has the
// bits of the fp32 call here on the widened tables -- both element types run the SAME <.., DROP> forms (no window form).
// On short rows most of a wave idles: a row of 5 edges fills 5 of the 16 (32) groups of ONE step.
#include "gatv2_seq.h"

namespace {

// M(G, H) for the kernel instance of a shape gat_narrow_shape() admits
#define GAIB_NARROW_DISPATCH(M)        \
  do {                                 \
    if (len == 16) {                   \
      if (heads == 1) M(4, 1);         \
      else if (heads == 2) M(4, 2);    \
      else M(4, 4);                    \
    } else {                           \
      if (heads == 1) M(2, 1);         \
      else M(2, 2);                    \
    }                                  \
  } while (0)

template <int G, int H, bool DROP, typename E>
void narrow_fwd_launch(gaib_ctx* ctx, const gaib_graph* g, unsigned grid, int per_xcd, const E* h, const float* alpha_l,
                       const float* alpha_r, float eps, float* out_partial, float2* ms_partial, const DropWin& dw) {
  gat_fwd_fused_chunk_kernel<G, H, G, E, DROP><<<grid, 256, 0, ctx->stream>>>(
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, 4 * G, h, alpha_l, alpha_r, eps, out_partial,
      ms_partial, -1, (uint32_t)g->nv, per_xcd, dw.rate, dw.scale, dw.seed);
}
// (RECOMP: the attention is formed again from the records; rev is read under DROP only)
template <int G, int H, bool DROP, typename E>
void narrow_bwd_launch(gaib_ctx* ctx, const gaib_graph* g, unsigned grid, int per_xcd, const E* feat, const E* grad, const f4* rec,
                       const float* alpha_l, const float* alpha_r, float eps, float* out_partial, float* rc_partial, const DropWin& dw) {
  gat_bwd_fused_chunk_kernel<G, H, G, true, E, DROP><<<grid, 256, 0, ctx->stream>>>(
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, g->rev, 4 * G, feat, grad, nullptr, nullptr,
      nullptr, alpha_l, alpha_r, eps, out_partial, rc_partial, rec, -1, (uint32_t)g->nv, 4 * G, H, per_xcd, dw.rate, dw.scale, dw.seed);
}
template <int G, int H, bool DROP, typename E>
void narrow_v2_fwd_launch(gaib_ctx* ctx, const gaib_graph* g, unsigned grid, int per_xcd, const E* h, const float* a, float eps,
                          float* out_partial, float2* ms_partial, const DropWin& dw) {
  gatv2_fwd_chunk_kernel<G, H, G, false, DROP, E><<<grid, 256, 0, ctx->stream>>>(
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, h, a, eps, out_partial, ms_partial, per_xcd, 4 * G,
      dw.rate, dw.scale, dw.seed, dw.mask_heads, dw.mask_head0);
}
template <int G, int H, bool DROP, typename E>
void narrow_v2_bwd_launch(gaib_ctx* ctx, const gaib_graph* g, unsigned grid, int per_xcd, const E* feat, const E* grad, const f4* rec,
                          const float* a, float eps, float* out_partial, float* agrad_partial, const DropWin& dw) {
  gatv2_bwd_chunk_kernel<G, H, G, false, DROP, E><<<grid, 256, 0, ctx->stream>>>(
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, feat, grad, rec, a, eps, out_partial,
      agrad_partial, per_xcd, 4 * G, g->rev, dw.rate, dw.scale, dw.seed, dw.mask_heads, dw.mask_head0);
}

// per row: the chunks' (m, s, acc) in chunk order -> out = act(sum / S) and row_stats = (M, 1 / S); rows without an edge: zeros
// and (-1e30, 0)
int narrow_fwd_reduce(gaib_ctx* ctx, const gaib_graph* g, int len, int heads, const float* out_partial, const float2* ms_partial,
                      int relu, float* out, float* row_stats) {
  float2* stats = reinterpret_cast<float2*>(row_stats);
  if (len == 16)
    gat_fwd_reduce_kernel<4><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, g->chunk_start, out_partial, ms_partial,
                                                                      relu ? 1 : 0, out, stats);
  else
    gat_fwd_reduce_kernel<2><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, g->chunk_start, out_partial, ms_partial,
                                                                      relu ? 1 : 0, out, stats);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}
// per row: the chunks' partial rows (and, H > 0, the row / column sums of g) in chunk order
int narrow_bwd_reduce(gaib_ctx* ctx, const gaib_graph* g, int len, int H, const float* out_partial, const float* rc_partial,
                      float* grad_out, float* rs, float* cs) {
  if (len == 16)
    gat_fused_reduce_kernel<4><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, H, g->chunk_start, out_partial, rc_partial, grad_out,
                                                                        rs, cs);
  else
    gat_fused_reduce_kernel<2><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, H, g->chunk_start, out_partial, rc_partial, grad_out,
                                                                        rs, cs);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

}  // namespace

// ---- GAT (static scores) ---------------------------------------------------------------------------------------------------------
template <typename E>
int gat_narrow_forward_run(gaib_ctx* ctx, const gaib_graph* g, int len, int heads, unsigned grid, int per_xcd, const E* h,
                           const float* alpha_l, const float* alpha_r, float eps, int relu, float* out_partial, float* ms_partial,
                           float* out, float* row_stats, const DropWin* drop) {
  GAIB_CHECK(gat_narrow_shape(len, heads), "gat_narrow_forward_run: len %d, heads %d", len, heads);
  const DropWin dw = drop ? *drop : DropWin{0.f, 1.f, 0, 0, 0};
  float2* ms = reinterpret_cast<float2*>(ms_partial);
#define GAIB_NF(GG, HH)                                                                                              \
  do {                                                                                                               \
    if (drop) narrow_fwd_launch<GG, HH, true, E>(ctx, g, grid, per_xcd, h, alpha_l, alpha_r, eps, out_partial, ms, dw); \
    else narrow_fwd_launch<GG, HH, false, E>(ctx, g, grid, per_xcd, h, alpha_l, alpha_r, eps, out_partial, ms, dw);  \
  } while (0)
  if (grid > 0) {
    GAIB_NARROW_DISPATCH(GAIB_NF);
    GAIB_LAUNCH_CHECK();
  }
#undef GAIB_NF
  return narrow_fwd_reduce(ctx, g, len, heads, out_partial, ms, relu, out, row_stats);
}

// the sweep over the records rec [nv][heads], then the rows' sums in chunk order: grad_out, rs and cs [nv][heads]
template <typename E>
int gat_narrow_backward_run(gaib_ctx* ctx, const gaib_graph* g, int len, int heads, unsigned grid, int per_xcd, const E* feat,
                            const E* grad, const float* rec, const float* alpha_l, const float* alpha_r, float eps, float* out_partial,
                            float* rc_partial, float* grad_out, float* rs, float* cs, const DropWin* drop) {
  GAIB_CHECK(gat_narrow_shape(len, heads), "gat_narrow_backward_run: len %d, heads %d", len, heads);
  GAIB_CHECK(!drop || g->rev, "gat_narrow_backward_run: the dropped sweep needs the reverse-edge permutation");
  const DropWin dw = drop ? *drop : DropWin{0.f, 1.f, 0, 0, 0};
  const f4* rec4 = reinterpret_cast<const f4*>(rec);
#define GAIB_NB(GG, HH)                                                                                                                  \
  do {                                                                                                                                   \
    if (drop) narrow_bwd_launch<GG, HH, true, E>(ctx, g, grid, per_xcd, feat, grad, rec4, alpha_l, alpha_r, eps, out_partial, rc_partial, dw); \
    else narrow_bwd_launch<GG, HH, false, E>(ctx, g, grid, per_xcd, feat, grad, rec4, alpha_l, alpha_r, eps, out_partial, rc_partial, dw); \
  } while (0)
  if (grid > 0) {
    GAIB_NARROW_DISPATCH(GAIB_NB);
    GAIB_LAUNCH_CHECK();
  }
#undef GAIB_NB
  return narrow_bwd_reduce(ctx, g, len, heads, out_partial, rc_partial, grad_out, rs, cs);
}

// ---- GATv2 -----------------------------------------------------------------------------------------------------------------------
template <typename E>
int gatv2_narrow_forward_run(gaib_ctx* ctx, const gaib_graph* g, int len, int heads, unsigned grid, int per_xcd, const E* h,
                             const float* a, float eps, int relu, float* out_partial, float* ms_partial, float* out, float* row_stats,
                             const DropWin* drop) {
  GAIB_CHECK(gat_narrow_shape(len, heads), "gatv2_narrow_forward_run: len %d, heads %d", len, heads);
  const DropWin dw = drop ? *drop : DropWin{0.f, 1.f, 0, 0, 0};
  float2* ms = reinterpret_cast<float2*>(ms_partial);
#define GAIB_NV2F(GG, HH)                                                                                    \
  do {                                                                                                       \
    if (drop) narrow_v2_fwd_launch<GG, HH, true, E>(ctx, g, grid, per_xcd, h, a, eps, out_partial, ms, dw);  \
    else narrow_v2_fwd_launch<GG, HH, false, E>(ctx, g, grid, per_xcd, h, a, eps, out_partial, ms, dw);      \
  } while (0)
  if (grid > 0) {
    GAIB_NARROW_DISPATCH(GAIB_NV2F);
    GAIB_LAUNCH_CHECK();
  }
#undef GAIB_NV2F
  return narrow_fwd_reduce(ctx, g, len, heads, out_partial, ms, relu, out, row_stats);
}

// the sweep, then the rows' sums in chunk order: grad_out; agrad_partial is left for the caller's two-level sum (v2_agrad)
template <typename E>
int gatv2_narrow_backward_run(gaib_ctx* ctx, const gaib_graph* g, int len, int heads, unsigned grid, int per_xcd, const E* feat,
                              const E* grad, const float* rec, const float* a, float eps, float* out_partial, float* agrad_partial,
                              float* grad_out, const DropWin* drop) {
  GAIB_CHECK(gat_narrow_shape(len, heads), "gatv2_narrow_backward_run: len %d, heads %d", len, heads);
  GAIB_CHECK(!drop || g->rev, "gatv2_narrow_backward_run: the dropped sweep needs the reverse-edge permutation");
  const DropWin dw = drop ? *drop : DropWin{0.f, 1.f, 0, 0, 0};
  const f4* rec4 = reinterpret_cast<const f4*>(rec);
#define GAIB_NV2B(GG, HH)                                                                                                          \
  do {                                                                                                                             \
    if (drop) narrow_v2_bwd_launch<GG, HH, true, E>(ctx, g, grid, per_xcd, feat, grad, rec4, a, eps, out_partial, agrad_partial, dw); \
    else narrow_v2_bwd_launch<GG, HH, false, E>(ctx, g, grid, per_xcd, feat, grad, rec4, a, eps, out_partial, agrad_partial, dw);  \
  } while (0)
  if (grid > 0) {
    GAIB_NARROW_DISPATCH(GAIB_NV2B);
    GAIB_LAUNCH_CHECK();
  }
#undef GAIB_NV2B
  // (H = 0: the row / column sums of the static scores have no part here, nothing of them is read or written)
  return narrow_bwd_reduce(ctx, g, len, 0, out_partial, nullptr, grad_out, nullptr, nullptr);
}

#define GAIB_NARROW_INSTANCES(E)                                                                                                      \
  template int gat_narrow_forward_run<E>(gaib_ctx*, const gaib_graph*, int, int, unsigned, int, const E*, const float*, const float*, \
                                         float, int, float*, float*, float*, float*, const DropWin*);                                 \
  template int gat_narrow_backward_run<E>(gaib_ctx*, const gaib_graph*, int, int, unsigned, int, const E*, const E*, const float*,    \
                                          const float*, const float*, float, float*, float*, float*, float*, float*, const DropWin*); \
  template int gatv2_narrow_forward_run<E>(gaib_ctx*, const gaib_graph*, int, int, unsigned, int, const E*, const float*, float, int, \
                                           float*, float*, float*, float*, const DropWin*);                                           \
  template int gatv2_narrow_backward_run<E>(gaib_ctx*, const gaib_graph*, int, int, unsigned, int, const E*, const E*, const float*,  \
                                            const float*, float, float*, float*, float*, const DropWin*)
GAIB_NARROW_INSTANCES(float);
GAIB_NARROW_INSTANCES(uint16_t);
#undef GAIB_NARROW_INSTANCES
