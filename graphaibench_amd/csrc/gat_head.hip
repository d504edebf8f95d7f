// gat_head.hip -- the one-sweep GAT for a single head of 256 or 512 columns on fp32 tables (option "gat_fused_head"): the shape
// rule and the launches of gat_head_kernels.h.  gaib_gat_forward_fused / gaib_gat_backward_fused reach them through the
// sequences of gat_fused_seq.h (gat_head_forward_seq / gat_head_backward_seq), which check the call, lay out the workspace as the
// narrow call's at width len, and run the narrow calls' own rowdot, record and alpha-gradient kernels around the sweep.
// Edges in flight per wave, chosen from the register report: forward 8 at 256 columns and 4 at 512, backward 4
// and 2 -- 32 row pieces of 16 bytes per lane in every case.
#include "gat_head_kernels.h"

// the shape rule (include/gaib.h): pure, no context, no device
extern "C" int gaib_gat_fused_head_cpl(int len, int heads) {
  if (heads != 1) return 0;
  return len == 256 ? 4 : len == 512 ? 8 : 0;
}

// chunk sweep, then the per-row combine: d_out = act(P h), d_row_stats [nv][stats_ld][2] = (M, 1 / S) of head 0
int gat_head_forward_run(gaib_ctx* ctx, const gaib_graph* g, int cpl, unsigned grid, int per_xcd, const float* h, int ld,
                         const float* alpha_l, const float* alpha_r, float eps, int relu, float* out_partial, float* ms_partial,
                         float* out, float* row_stats, int stats_ld) {
  float2* ms = reinterpret_cast<float2*>(ms_partial);
  float2* stats = reinterpret_cast<float2*>(row_stats);
#define GAIB_HF(CPL, U)                                                                                                              \
  do {                                                                                                                               \
    gat_head_fwd_chunk_kernel<CPL, U><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start,       \
                                                                     g->rowptr, g->colidx, h, ld, alpha_l, alpha_r, eps, out_partial, \
                                                                     ms, per_xcd);                                                   \
    GAIB_LAUNCH_CHECK();                                                                                                             \
    gat_head_fwd_reduce_kernel<CPL><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, g->chunk_start, out_partial, ms, relu ? 1 : 0,   \
                                                                             out, ld, stats, stats_ld);                              \
  } while (0)
  if (cpl == 4) GAIB_HF(4, 8);
  else GAIB_HF(8, 4);
#undef GAIB_HF
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// chunk sweep over the records rec [nv][rec_ld], then the rows' sums in chunk order: d_grad_out, rs and cs [nv]
int gat_head_backward_run(gaib_ctx* ctx, const gaib_graph* g, int cpl, unsigned grid, int per_xcd, const float* feat,
                          const float* grad, int ld, const float* rec, int rec_ld, const float* alpha_l, const float* alpha_r,
                          float eps, float* out_partial, float* rc_partial, float* grad_out, float* rs, float* cs) {
  const f4* rec4 = reinterpret_cast<const f4*>(rec);
#define GAIB_HB(CPL, U)                                                                                                              \
  do {                                                                                                                               \
    gat_head_bwd_chunk_kernel<CPL, U><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start,       \
                                                                     g->rowptr, g->colidx, feat, grad, ld, rec4, rec_ld, alpha_l,    \
                                                                     alpha_r, eps, out_partial, rc_partial, per_xcd);                \
    GAIB_LAUNCH_CHECK();                                                                                                             \
    gat_head_bwd_reduce_kernel<CPL><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, g->chunk_start, out_partial, rc_partial,         \
                                                                             grad_out, ld, rs, cs);                                  \
  } while (0)
  if (cpl == 4) GAIB_HB(4, 4);
  else GAIB_HB(8, 2);
#undef GAIB_HB
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}
