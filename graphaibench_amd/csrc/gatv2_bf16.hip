// gatv2_bf16.hip -- the one-sweep GATv2 over bf16 tables (options "gat_v2" and "gat_bf16" of the layer library together): the
// sequences of gatv2_seq.h on the element type E = uint16_t, plain and under attention dropout, narrow and -- with option
// gatv2_wide -- on column slabs and on one head of 256 or 512 columns (that head's bf16 kernels are gatv2_head.hip's).
// Every read of h and grad -- the chunk's own rows h_i and g_i, the gathered rows, grad in the row dots <g_v, out_v> of the
// prologue, h wherever a's gradient reads phi(h_j + h_i) -- takes raw bf16 bits (a lane's four columns of a row are one 8-byte
// load) and widens them exactly (a shift / a mask), the gathered rows on the consume side of the batch's sched_barrier; everything
// behind the widening is the fp32 kernel's text, lane map and order of sums.  So every output has the bits of the corresponding
// fp32 call on the tables widened to fp32, under the same options (gat_chunk_xcd, gatv2_wide) and the same (rate, scale, seed): the
// function is fp32 GATv2 on the rounded table, and the backward the exact gradient of that forward.  z = h_i + h_j is formed from
// widened values and stays commutative bit for bit: the score is symmetric as in fp32, which the single backward sweep rests on.
// A gathered row is 2 len bytes instead of 4 len.  Cover and refusals are the fp32 calls' (the 4 GB bound on nv len 4 included);
// the bf16 tables must be 8-byte aligned, the other buffers 16.  Profile: the fp32 calls' keys and byte formulas (a work rate in
// dense bytes).
#include "gatv2_seq.h"

extern "C" int gaib_gatv2_forward_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_h_bf16, const float* d_a,
                                       float eps, int relu, float* d_out, float* d_row_stats) {
  return v2_forward_seq<uint16_t>("gaib_gatv2_forward_bf16", ctx, g, len, heads, d_h_bf16, d_a, eps, relu, d_out, d_row_stats, nullptr);
}

extern "C" int gaib_gatv2_backward_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_feat_bf16,
                                        const uint16_t* d_grad_bf16, const float* d_fwd_out, const float* d_a, const float* d_row_stats,
                                        float eps, float* d_grad_out, float* d_a_grad) {
  return v2_backward_seq<uint16_t>("gaib_gatv2_backward_bf16", ctx, g, len, heads, d_feat_bf16, d_grad_bf16, d_fwd_out, d_a,
                                   d_row_stats, eps, d_grad_out, d_a_grad, nullptr);
}

extern "C" int gaib_gatv2_forward_drop_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_h_bf16,
                                            const float* d_a, float eps, int relu, float drop_rate, float scale, uint64_t seed,
                                            float* d_out, float* d_row_stats) {
  const DropWin dw = {drop_rate, scale, seed, heads, 0};
  return v2_forward_seq<uint16_t>("gaib_gatv2_forward_drop_bf16", ctx, g, len, heads, d_h_bf16, d_a, eps, relu, d_out, d_row_stats, &dw);
}

extern "C" int gaib_gatv2_backward_drop_bf16(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const uint16_t* d_feat_bf16,
                                             const uint16_t* d_grad_bf16, const float* d_fwd_out, const float* d_a,
                                             const float* d_row_stats, float eps, float drop_rate, float scale, uint64_t seed,
                                             float* d_grad_out, float* d_a_grad) {
  const DropWin dw = {drop_rate, scale, seed, heads, 0};
  return v2_backward_seq<uint16_t>("gaib_gatv2_backward_drop_bf16", ctx, g, len, heads, d_feat_bf16, d_grad_bf16, d_fwd_out, d_a,
                                   d_row_stats, eps, d_grad_out, d_a_grad, &dw);
}
