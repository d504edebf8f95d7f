// gat_fused.hip -- the one-sweep GAT on fp32 tables: every public entry point, each a few lines that name the call's arguments
// for the sequences of gat_fused_seq.h (which see for the instantiation every call reaches).
//   gaib_gat_forward_fused / gaib_gat_backward_fused             whole graphs; backward from the attention array or the row statistics
//   gaib_gat_forward_fused_rect / gaib_gat_backward_fused_rect   a rank's rectangular graph, in phases (gaib_gat_backward_rec: its records)
//   gaib_gat_*_fused_drop                                        attention dropout inside the sweeps (option "gat_fused_drop" of the layers)
//   gaib_gat_*_fused_drop_win                                    the same with the mask's head window named by the caller
//   gaib_gat_fused_slabs                                         the shape rule of option "gat_fused_wide"
// Forward (gat_fwd_fused_chunk_kernel): d_out = act(P h) and d_row_stats [nv][heads][2] = (row maximum of the leaky-relu'd scores,
// 1 / row sum of exp) -- everything backward needs to form the attention again; no [ne][heads] array is written.  Where a call does
// not apply (shape, graph, alignment, option "gat_fused_fwd" / "gat_fused_bwd" = 0) it returns GAIB_ERR_UNSUPPORTED with nothing
// touched, and the caller runs the staged entry points of gat.hip.
// Attention dropout: the mask of (edge e, head k) is the one gaib_dropout draws for element e * heads + k of an [ne][heads] array
// under the same seed, formed inside the sweep (gat_drop_bits) -- no [ne][heads] array exists on this path either.
//   forward:  out_i = act(sum_e p_e w_e h_c), w = mask . scale; the softmax and so d_row_stats do not see the mask
//   backward: dp_e = w_e <grad_i, h_c>, dp_r = w_r <grad_c, h_i>, out_i += p_r w_r grad_c with r = rev(e); rowdot_v = <grad_v, out_v>
//             is still sum_e p_e dp_e of row v with the dropped output, so the records and everything after the sweep are those of
//             gaib_gat_backward_fused (row-statistics form)
// With rate 0 and scale 1 every w is 1.0f and a product by it changes no bit: the results are the undropped calls'.  The reverse
// edge's mask needs rev(e): a graph without a reverse-edge permutation is refused by forward and backward alike.
// Options: gat_chunk_xcd and gat_fused_unroll everywhere but in _rect; gat_bwd_pk and gat_interleave in the narrow undropped
// row-statistics backward only.  Deterministic, no atomics.
#include "gat_fused_seq.h"

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

extern "C" int gaib_gat_forward_fused(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h,
                                      const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu,
                                      float* d_out, float* d_row_stats) {
  const GatFwd<float> a = {"gaib_gat_forward_fused", len, heads, d_h, d_alpha_l, d_alpha_r, epsilon, relu, d_out, d_row_stats};
  return gat_forward_fused_seq(ctx, g, a);
}

// the same on a rank's RECTANGULAR graph (rows = owned vertices, columns = [owned | halo]): d_tab [nc x len] holds the owned
// rows of h first, then the halo rows.  phase: -1 = the whole sweep + the per-row combination (a table that is complete);
// 0 = only the chunks over owned columns (columns < g->nv), nothing else -- it may run while the halo rows are still arriving;
// 1 = the remaining chunks + the combination.  The partial results of phase 0 live in the context's workspace until phase 1:
// no other call on the context in between.
extern "C" int gaib_gat_forward_fused_rect(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_tab,
                                           const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu,
                                           float* d_out, float* d_row_stats, int phase) {
  GatFwd<float> a = {"gaib_gat_forward_fused_rect", len, heads, d_tab, d_alpha_l, d_alpha_r, epsilon, relu, d_out, d_row_stats};
  a.phase = phase, a.rect = true;
  return gat_forward_fused_seq(ctx, g, a);
}

extern "C" int gaib_gat_backward_fused(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat,
                                       const float* d_grad, const float* d_fwd_out, const float* d_alpha_l,
                                       const float* d_alpha_r, const float* d_norm_scores, const float* d_row_stats,
                                       float epsilon, float* d_grad_out, float* d_alpha_lgrad, float* d_alpha_rgrad) {
  const GatBwd<float> a = {"gaib_gat_backward_fused", len, heads, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r, d_norm_scores,
                           d_row_stats, nullptr, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad};
  return gat_backward_fused_seq(ctx, g, a);
}

// ---- the one-sweep backward on a rank's RECTANGULAR graph ----------------------------------------------------------------------------
// Everything row i needs about its edge (i -> c) and the reverse edge (c -> i) follows from per-VERTEX quantities of i and
// c (h, grad, and the record (rowdot, row maximum, 1 / row sum)), and in a structurally symmetric graph the in-edges of i
// are the reverses of its out-edges: so the rank that owns row i computes rs_i, cs_i and the aggregated gradient of i from
// i's own edge list alone, given the halo vertices' h rows (still there from forward), grad rows and records.  No
// transposed structure, no permuted [ne][H] copies, no reverse exchange of partial rows: two forward-direction halo
// exchanges (grad rows, records) and one sweep.
//   gaib_gat_backward_rec: the owned vertices' records  rec[v][h] = (<grad_v, out_v>_h, M_vh, 1/S_vh, 0)
//   gaib_gat_backward_fused_rect: d_feat_tab / d_grad_tab [nc x len], d_rec_tab [nc][heads][4] with the owned rows first;
//     phase as in gaib_gat_forward_fused_rect (0 reads owned rows only).  The alpha gradients cover the OWNED rows: the
//     caller sums them over the ranks.
extern "C" int gaib_gat_backward_rec(gaib_ctx* ctx, int64_t nv, int len, int heads, const float* d_grad, const float* d_fwd_out,
                                     const float* d_row_stats, float* d_rec) {
  GAIB_CHECK(ctx && (nv == 0 || (d_grad && d_fwd_out && d_row_stats && d_rec)), "gaib_gat_backward_rec: NULL argument");
  GAIB_TRY(check_heads("gaib_gat_backward_rec", len, heads));
  if (nv <= 0) return GAIB_OK;
  GAIB_HIP(hipSetDevice(ctx->device));
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * up4((size_t)nv * heads)));
  return gat_bwd_prologue<float, false>(ctx, nv, len, heads, len, heads, d_grad, d_fwd_out, d_row_stats, (float*)ctx->ws,
                                        reinterpret_cast<f4*>(d_rec));
}

extern "C" int gaib_gat_backward_fused_rect(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat_tab,
                                            const float* d_grad_tab, const float* d_rec_tab, const float* d_alpha_l,
                                            const float* d_alpha_r, float epsilon, float* d_grad_out, float* d_alpha_lgrad,
                                            float* d_alpha_rgrad, int phase) {
  GatBwd<float> a = {"gaib_gat_backward_fused_rect", len, heads, d_feat_tab, d_grad_tab, nullptr, d_alpha_l, d_alpha_r, nullptr,
                     nullptr, d_rec_tab, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad};
  a.phase = phase, a.rect = true;
  return gat_backward_fused_seq(ctx, g, a);
}

// ---- attention dropout -----------------------------------------------------------------------------------------------------------------
extern "C" int gaib_gat_forward_fused_drop(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h, const float* d_alpha_l,
                                           const float* d_alpha_r, float epsilon, int relu, float drop_rate, float scale, uint64_t seed,
                                           float* d_out, float* d_row_stats) {
  const DropWin drop = {drop_rate, scale, seed, heads, 0};
  GatFwd<float> a = {"gaib_gat_forward_fused_drop", len, heads, d_h, d_alpha_l, d_alpha_r, epsilon, relu, d_out, d_row_stats};
  a.drop = &drop;
  return gat_forward_fused_seq(ctx, g, a);
}

extern "C" int gaib_gat_backward_fused_drop(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat, const float* d_grad,
                                            const float* d_fwd_out, const float* d_alpha_l, const float* d_alpha_r,
                                            const float* d_row_stats, float epsilon, float drop_rate, float scale, uint64_t seed,
                                            float* d_grad_out, float* d_alpha_lgrad, float* d_alpha_rgrad) {
  const DropWin drop = {drop_rate, scale, seed, heads, 0};
  GatBwd<float> a = {"gaib_gat_backward_fused_drop", len, heads, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r, nullptr,
                     d_row_stats, nullptr, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad};
  a.drop = &drop;
  return gat_backward_fused_seq(ctx, g, a);
}

// the window sequence at a narrow shape, contiguous tables (include/gaib.h): one slab with ld = len, stats_ld = heads -- the unit a
// wide dropped call is made of
extern "C" int gaib_gat_forward_fused_drop_win(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_h,
                                               const float* d_alpha_l, const float* d_alpha_r, float epsilon, int relu,
                                               float drop_rate, float scale, uint64_t seed, int mask_heads, int mask_head0,
                                               float* d_out, float* d_row_stats) {
  const DropWin drop = {drop_rate, scale, seed, mask_heads, mask_head0};
  GatFwd<float> a = {"gaib_gat_forward_fused_drop_win", len, heads, d_h, d_alpha_l, d_alpha_r, epsilon, relu, d_out, d_row_stats};
  a.drop = &drop, a.win = true;
  return gat_forward_fused_seq(ctx, g, a);
}

extern "C" int gaib_gat_backward_fused_drop_win(gaib_ctx* ctx, gaib_graph* g, int len, int heads, const float* d_feat,
                                                const float* d_grad, const float* d_fwd_out, const float* d_alpha_l,
                                                const float* d_alpha_r, const float* d_row_stats, float epsilon, float drop_rate,
                                                float scale, uint64_t seed, int mask_heads, int mask_head0, float* d_grad_out,
                                                float* d_alpha_lgrad, float* d_alpha_rgrad) {
  const DropWin drop = {drop_rate, scale, seed, mask_heads, mask_head0};
  GatBwd<float> a = {"gaib_gat_backward_fused_drop_win", len, heads, d_feat, d_grad, d_fwd_out, d_alpha_l, d_alpha_r, nullptr,
                     d_row_stats, nullptr, epsilon, d_grad_out, d_alpha_lgrad, d_alpha_rgrad};
  a.drop = &drop, a.win = true;
  return gat_backward_fused_seq(ctx, g, a);
}
