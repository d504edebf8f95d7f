// gatv2.hip -- the one-sweep GATv2 on fp32 tables (include/gaib.h: gaib_gatv2_forward / gaib_gatv2_backward and their _drop forms):
// the sequences of gatv2_seq.h on the element type E = float.  The file comment there has the cover, the slabs, the single wide head
// and attention dropout; gatv2_bf16.hip holds the same four calls over bf16 tables.
#include "gatv2_seq.h"

extern "C" int gaib_gatv2_forward(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h, const float* d_a, float eps,
                                  int relu, float* d_out, float* d_row_stats) {
  return v2_forward_seq<float>("gaib_gatv2_forward", ctx, g, len, heads, d_h, d_a, eps, relu, d_out, d_row_stats, nullptr);
}

extern "C" int gaib_gatv2_backward(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat, const float* d_grad,
                                   const float* d_fwd_out, const float* d_a, const float* d_row_stats, float eps, float* d_grad_out,
                                   float* d_a_grad) {
  return v2_backward_seq<float>("gaib_gatv2_backward", ctx, g, len, heads, d_feat, d_grad, d_fwd_out, d_a, d_row_stats, eps, d_grad_out,
                                d_a_grad, nullptr);
}

extern "C" int gaib_gatv2_forward_drop(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h, const float* d_a, float eps,
                                       int relu, float drop_rate, float scale, uint64_t seed, float* d_out, float* d_row_stats) {
  const DropWin dw = {drop_rate, scale, seed, heads, 0};
  return v2_forward_seq<float>("gaib_gatv2_forward_drop", ctx, g, len, heads, d_h, d_a, eps, relu, d_out, d_row_stats, &dw);
}

extern "C" int gaib_gatv2_backward_drop(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat, const float* d_grad,
                                        const float* d_fwd_out, const float* d_a, const float* d_row_stats, float eps, float drop_rate,
                                        float scale, uint64_t seed, float* d_grad_out, float* d_a_grad) {
  const DropWin dw = {drop_rate, scale, seed, heads, 0};
  return v2_backward_seq<float>("gaib_gatv2_backward_drop", ctx, g, len, heads, d_feat, d_grad, d_fwd_out, d_a, d_row_stats, eps,
                                d_grad_out, d_a_grad, &dw);
}
