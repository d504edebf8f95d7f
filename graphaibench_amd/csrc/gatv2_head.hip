// gatv2_head.hip -- the one-sweep GATv2 for a single head of 256 or 512 columns (option "gatv2_wide"): the launches of
// gatv2_head_kernels.h, on fp32 tables and on bf16 tables (E = uint16_t, raw bits).  The GATv2 calls (gatv2_seq.h) check the call,
// lay out the workspace as the narrow call's at (len, 1) and run the narrow call's own rowdot, record and a-gradient kernels around
// the sweep.  Every GATv2 head kernel is instantiated here and nowhere else (gatv2.hip and gatv2_bf16.hip link against the two
// explicit instantiations below).
// Edges in flight per wave, from the register report: forward 8 at 256 columns and 4 at 512, backward
// 4 and 2 -- 32 row pieces per lane in every case, the static-score head sweeps' values -- with and without attention dropout (the
// masks are two scalar pairs), on fp32 and on bf16 tables (packed pieces wait in half the registers; the batch is not lengthened,
// as in gat_head.hip).
#include "gatv2_head_kernels.h"

namespace {

template <int CPL, int U, bool DROP, typename E>
void v2_head_fwd_launch(gaib_ctx* ctx, const gaib_graph* g, unsigned grid, int per_xcd, const E* h, const float* a, float eps,
                        float* out_partial, float2* ms_partial, const DropWin& dw) {
  gatv2_head_fwd_chunk_kernel<CPL, U, DROP, E><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start,
                                                                              g->rowptr, g->colidx, h, a, eps, out_partial, ms_partial,
                                                                              per_xcd, dw.rate, dw.scale, dw.seed);
}
template <int CPL, int U, bool DROP, typename E>
void v2_head_bwd_launch(gaib_ctx* ctx, const gaib_graph* g, unsigned grid, int per_xcd, const E* feat, const E* grad, const f4* rec,
                        const float* a, float eps, float* out_partial, float* agrad_partial, const DropWin& dw) {
  gatv2_head_bwd_chunk_kernel<CPL, U, DROP, E><<<grid, 256, 0, ctx->stream>>>(g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start,
                                                                              g->rowptr, g->colidx, feat, grad, rec, a, eps,
                                                                              out_partial, agrad_partial, per_xcd, g->rev, dw.rate,
                                                                              dw.scale, dw.seed);
}

}  // namespace

// chunk sweep, then the per-row combine: out = act(P h), row_stats [nv][2] = (m, 1 / l)
template <typename E>
int gatv2_head_forward_run(gaib_ctx* ctx, const gaib_graph* g, int cpl, unsigned grid, int per_xcd, const E* h, const float* a,
                           float eps, int relu, float* out_partial, float2* ms_partial, float* out, float* row_stats,
                           const DropWin* drop) {
  const DropWin dw = drop ? *drop : DropWin{0.f, 1.f, 0, 0, 0};
#define GAIB_V2HF(CPL, U)                                                                                                            \
  do {                                                                                                                               \
    if (grid > 0) {                                                                                                                  \
      if (drop) v2_head_fwd_launch<CPL, U, true, E>(ctx, g, grid, per_xcd, h, a, eps, out_partial, ms_partial, dw);                  \
      else v2_head_fwd_launch<CPL, U, false, E>(ctx, g, grid, per_xcd, h, a, eps, out_partial, ms_partial, dw);                      \
      GAIB_LAUNCH_CHECK();                                                                                                           \
    }                                                                                                                                \
    gat_head_fwd_reduce_kernel<CPL><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, g->chunk_start, out_partial, ms_partial,         \
                                                                             relu ? 1 : 0, out, 64 * CPL,                            \
                                                                             reinterpret_cast<float2*>(row_stats), 1);               \
  } while (0)
  if (cpl == 4) GAIB_V2HF(4, 8);
  else GAIB_V2HF(8, 4);
#undef GAIB_V2HF
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// chunk sweep over the records rec [nv], then the rows' sums in chunk order: grad_out; agrad_partial [grid][len] is left for the
// caller's two-level sum
template <typename E>
int gatv2_head_backward_run(gaib_ctx* ctx, const gaib_graph* g, int cpl, unsigned grid, int per_xcd, const E* feat, const E* grad,
                            const f4* rec, const float* a, float eps, float* out_partial, float* agrad_partial, float* grad_out,
                            const DropWin* drop) {
  const DropWin dw = drop ? *drop : DropWin{0.f, 1.f, 0, 0, 0};
#define GAIB_V2HB(CPL, U)                                                                                                            \
  do {                                                                                                                               \
    if (grid > 0) {                                                                                                                  \
      if (drop) v2_head_bwd_launch<CPL, U, true, E>(ctx, g, grid, per_xcd, feat, grad, rec, a, eps, out_partial, agrad_partial, dw); \
      else v2_head_bwd_launch<CPL, U, false, E>(ctx, g, grid, per_xcd, feat, grad, rec, a, eps, out_partial, agrad_partial, dw);     \
      GAIB_LAUNCH_CHECK();                                                                                                           \
    }                                                                                                                                \
    gatv2_head_rows_kernel<CPL><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, g->chunk_start, out_partial, grad_out);              \
  } while (0)
  if (cpl == 4) GAIB_V2HB(4, 4);
  else GAIB_V2HB(8, 2);
#undef GAIB_V2HB
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

#define GAIB_V2_HEAD_INSTANCES(E)                                                                                                    \
  template int gatv2_head_forward_run<E>(gaib_ctx*, const gaib_graph*, int, unsigned, int, const E*, const float*, float, int,       \
                                         float*, float2*, float*, float*, const DropWin*);                                           \
  template int gatv2_head_backward_run<E>(gaib_ctx*, const gaib_graph*, int, unsigned, int, const E*, const E*, const f4*,           \
                                          const float*, float, float*, float*, float*, const DropWin*)
GAIB_V2_HEAD_INSTANCES(float);
GAIB_V2_HEAD_INSTANCES(uint16_t);
#undef GAIB_V2_HEAD_INSTANCES
