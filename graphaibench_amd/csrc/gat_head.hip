// gat_head.hip -- the one-sweep GAT for a single head of 256 or 512 columns (option "gat_fused_head"): the shape rule and the
// launches of gat_head_kernels.h, on fp32 tables and on bf16 tables (E = uint16_t, raw bits), plain and under attention dropout
// (options "gat_bf16" and "gat_fused_drop" next to "gat_fused_head": gat_head_route).  The public calls reach them through the
// sequences of gat_fused_seq.h (gat_head_forward_seq / gat_head_backward_seq), which check the call, lay out the workspace as the
// narrow call's at width len, and run the narrow calls' own rowdot, record and alpha-gradient kernels around the sweep.  Every
// head kernel is instantiated here and nowhere else (gat_bf16.hip links against the two explicit instantiations below).
// Edges in flight per wave, chosen from the register report: on fp32 tables forward 8 at 256 columns and 4 at 512,
// backward 4 and 2 -- 32 row pieces of 16 bytes per lane in every case.  The bf16 and the dropped forms keep those four values:
// packed rows wait in half the registers, but twice the edges in flight cost every bf16 kernel a wave of occupancy against its
// fp32 form (the address arithmetic and the widened copies of a longer batch), and as they are the bf16 forms run at the fp32
// forms' occupancy or above it.
#include "gat_head_kernels.h"

// the shape rule (include/gaib.h): pure, no context, no device
extern "C" int gaib_gat_fused_head_cpl(int len, int heads) {
  if (heads != 1) return 0;
  return len == 256 ? 4 : len == 512 ? 8 : 0;
}

// chunk sweep, then the per-row combine: d_out = act(P h), d_row_stats [nv][stats_ld][2] = (M, 1 / S) of head 0
template <typename E>
int gat_head_forward_run(gaib_ctx* ctx, const gaib_graph* g, int cpl, unsigned grid, int per_xcd, const E* h, int ld,
                         const float* alpha_l, const float* alpha_r, float eps, int relu, float* out_partial, float* ms_partial,
                         float* out, float* row_stats, int stats_ld, const DropWin* drop) {
  float2* ms = reinterpret_cast<float2*>(ms_partial);
  float2* stats = reinterpret_cast<float2*>(row_stats);
  // (the undropped launches leave the trailing arguments to their defaults)
#define GAIB_HF(CPL, U)                                                                                                              \
  do {                                                                                                                               \
    if (drop)                                                                                                                        \
      gat_head_fwd_chunk_kernel<CPL, U, E, true><<<grid, 256, 0, ctx->stream>>>(                                                     \
          g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, h, ld, alpha_l, alpha_r, eps, out_partial, \
          ms, per_xcd, drop->rate, drop->scale, drop->seed);                                                                         \
    else                                                                                                                             \
      gat_head_fwd_chunk_kernel<CPL, U, E><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, \
                                                                          g->rowptr, g->colidx, h, ld, alpha_l, alpha_r, eps,        \
                                                                          out_partial, ms, per_xcd);                                 \
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
template <typename E>
int gat_head_backward_run(gaib_ctx* ctx, const gaib_graph* g, int cpl, unsigned grid, int per_xcd, const E* feat, const E* grad,
                          int ld, const float* rec, int rec_ld, const float* alpha_l, const float* alpha_r, float eps,
                          float* out_partial, float* rc_partial, float* grad_out, float* rs, float* cs, const DropWin* drop) {
  const f4* rec4 = reinterpret_cast<const f4*>(rec);
  GAIB_CHECK(!drop || g->rev, "gat_head_backward_run: the dropped sweep needs the reverse-edge permutation");
#define GAIB_HB(CPL, U)                                                                                                              \
  do {                                                                                                                               \
    if (drop)                                                                                                                        \
      gat_head_bwd_chunk_kernel<CPL, U, E, true><<<grid, 256, 0, ctx->stream>>>(                                                     \
          g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, feat, grad, ld, rec4, rec_ld, alpha_l,    \
          alpha_r, eps, out_partial, rc_partial, per_xcd, g->rev, drop->rate, drop->scale, drop->seed);                              \
    else                                                                                                                             \
      gat_head_bwd_chunk_kernel<CPL, U, E><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, \
                                                                          g->rowptr, g->colidx, feat, grad, ld, rec4, rec_ld,        \
                                                                          alpha_l, alpha_r, eps, out_partial, rc_partial, per_xcd);  \
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

#define GAIB_HEAD_INSTANCES(E)                                                                                                       \
  template int gat_head_forward_run<E>(gaib_ctx*, const gaib_graph*, int, unsigned, int, const E*, int, const float*, const float*,  \
                                       float, int, float*, float*, float*, float*, int, const DropWin*);                             \
  template int gat_head_backward_run<E>(gaib_ctx*, const gaib_graph*, int, unsigned, int, const E*, const E*, int, const float*, int, \
                                        const float*, const float*, float, float*, float*, float*, float*, float*, const DropWin*)
GAIB_HEAD_INSTANCES(float);
GAIB_HEAD_INSTANCES(uint16_t);
#undef GAIB_HEAD_INSTANCES
