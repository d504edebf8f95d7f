// gat_bf16.hip -- the one-sweep GAT over bf16 tables (option "gat_bf16" of the layer library): the sequences of gat_fused_seq.h on
// the element type E = uint16_t, plain and under attention dropout (gaib_gat_*_fused_drop_bf16), narrow and -- with option
// gat_fused_wide -- on multi-head rows wider than 128 columns.
// Every read of h and grad -- own rows and gathered rows in the sweeps, grad in rowdot, h in the alpha gradients -- takes raw bf16
// bits (a lane's four columns of a row are one 8-byte load) and widens them exactly (a shift / a mask), on the consume side of the
// batch's sched_barrier; everything behind the widening is the fp32 kernel's text.  So every output has the bits of the
// corresponding fp32 call on the tables widened to fp32, under the same options and the same (rate, scale, seed).  A gathered row
// is 2 len bytes instead of 4 len: at 8 heads x 8 the backward sweep touches three 128-byte lines per edge (h, grad, records)
// instead of five.  Slab s gathers from column s w of the tables with the row stride len: 2 s w bytes, a multiple of 64 for every
// slab width, so the 8-byte loads stay aligned.
// Options: as the fp32 calls (gat_fused.hip), except that gat_interleave is ignored: the bf16 rows are gathered from their own
// tables, which changes no bits in fp32 either.  Profile: the fp32 calls' keys and byte formulas (a work rate in dense bytes).
#include "gat_fused_seq.h"

extern "C" int gaib_gat_forward_fused_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_h_bf16,
                                           const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu,
                                           float* d_out, float* d_row_stats) {
  const GatFwd<uint16_t> a = {"gaib_gat_forward_fused_bf16", len, heads, d_h_bf16, d_alpha_l, d_alpha_r, epsilon, relu, d_out, d_row_stats};
  return gat_forward_fused_seq(ctx, g, a);
}

extern "C" int gaib_gat_backward_fused_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_feat_bf16,
                                            const uint16_t* d_grad_bf16, const float* d_fwd_out, const float* d_alpha_l,
                                            const float* d_alpha_r, const float* d_row_stats, float epsilon, float* d_grad_out,
                                            float* d_alpha_lgrad, float* d_alpha_rgrad) {
  const GatBwd<uint16_t> a = {"gaib_gat_backward_fused_bf16", len, heads, d_feat_bf16, d_grad_bf16, d_fwd_out, d_alpha_l, d_alpha_r,
                              nullptr, d_row_stats, nullptr, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad};
  return gat_backward_fused_seq(ctx, g, a);
}

// attention dropout on bf16 tables (include/gaib.h); at a narrow shape the window form with the window (heads, 0)
extern "C" int gaib_gat_forward_fused_drop_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_h_bf16,
                                                const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu,
                                                float drop_rate, float scale, uint64_t seed, float* d_out, float* d_row_stats) {
  const DropWin drop = {drop_rate, scale, seed, heads, 0};
  GatFwd<uint16_t> a = {"gaib_gat_forward_fused_drop_bf16", len, heads, d_h_bf16, d_alpha_l, d_alpha_r, epsilon, relu, d_out, d_row_stats};
  a.drop = &drop;
  return gat_forward_fused_seq(ctx, g, a);
}

extern "C" int gaib_gat_backward_fused_drop_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_feat_bf16,
                                                 const uint16_t* d_grad_bf16, const float* d_fwd_out, const float* d_alpha_l,
                                                 const float* d_alpha_r, const float* d_row_stats, float epsilon, float drop_rate,
                                                 float scale, uint64_t seed, float* d_grad_out, float* d_alpha_lgrad,
                                                 float* d_alpha_rgrad) {
  const DropWin drop = {drop_rate, scale, seed, heads, 0};
  GatBwd<uint16_t> a = {"gaib_gat_backward_fused_drop_bf16", len, heads, d_feat_bf16, d_grad_bf16, d_fwd_out, d_alpha_l, d_alpha_r,
                        nullptr, d_row_stats, nullptr, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad};
  a.drop = &drop;
  return gat_backward_fused_seq(ctx, g, a);
}
