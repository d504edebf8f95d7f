// gatv2_seq.h -- the host side of the one-sweep GATv2, once: argument checks, workspace and the launch sequences around the two
// sweeps of gatv2_kernels.h, templated on the element type E of the gathered tables (float: gatv2.hip; uint16_t = raw bf16 bits:
// gatv2_bf16.hip).  Only the tables (h; feat and grad) have the type E; a, the records, statistics, partial sums and every output
// are fp32.
//   forward:   chunk grid (+ XCD walk), gatv2_fwd_chunk_kernel, gat_fwd_reduce_kernel (the v1 partial format: its kernel)
//   backward:  rowdot_kernel, gat_rec_kernel (records (delta, m, 1 / l)), gatv2_bwd_chunk_kernel, gat_fused_reduce_kernel (the
//              partial rows in chunk order), gatv2_agrad_strip_kernel, gatv2_agrad_final_kernel (a's gradient, two fixed levels)
// Cover: gat_fused_shape(len, heads) on whole graphs, tables whose fp32 form is below 4 GB (the sweeps address a row by a 32-bit
// byte offset; the bound is nv len 4 for both element types, so the fp32 and the bf16 call always decide alike).
// With option gatv2_wide = 1 (gatv2_route) also
//   * every multi-head row gaib_gat_fused_slabs cuts into S >= 2 column slabs of w columns and Hs = heads / S heads: the sequence
//     above once per slab, on the column window [s w, (s + 1) w) and the head window [s Hs, (s + 1) Hs) of the caller's arrays IN
//     PLACE (the <.., WIDE> sweeps and the WIDE rowdot, record and row-reduction kernels of gat_kernels.h / gat_fused_seq.h, row
//     strides len and heads).  The workspace is at the slab's width and the next slab reuses it (same stream).  Heads are
//     independent, and the chunk list, the grid and the strips of a's gradient follow from the graph alone: every output of slab s
//     has the BITS of the narrow call at (w, Hs) on contiguous copies of its windows.  Slab s of a bf16 table starts 2 s w bytes
//     into a row, a multiple of 64 for every slab width: the 8-byte loads stay aligned;
//   * one head of 256 or 512 columns (gaib_gat_fused_head_cpl): the sweeps of gatv2_head.hip between the narrow call's rowdot,
//     record and a-gradient kernels at (len, 1).
// With option gat_fused_narrow = 1 also rows of 16 columns (1, 2 or 4 heads) and 8 columns (1 or 2 heads): the same two sweeps at
// G = 4, 2 with the whole chunk as one batch, instantiated by gat_narrow.hip, between this file's prologue and a-gradient kernels.
// ATTENTION DROPOUT (the _drop calls): the SAME two host sequences with the sweeps' DROP instantiations -- the undropped calls are
// those sequences with drop = NULL.  The masks are formed inside the sweeps (no [ne][heads] array); slab s passes the head window
// (heads, s Hs) of the full row's mask array; the backward reads g->rev for the reverse edges' masks, and the forward asks for
// the permutation too so that both calls decide alike.
// The narrow call launches what it launched without the option.  There is NO staged GATv2: outside the cover the calls return
// GAIB_ERR_UNSUPPORTED with nothing touched and the caller has to say so.  Option gat_chunk_xcd is honoured.  Deterministic, no
// atomics.
#pragma once
#include "gat_fused_seq.h"
#include "gatv2_head_kernels.h"
#include "gatv2_kernels.h"

namespace {

// how a call runs: S slabs of w columns and Hs heads (S = 1: the narrow call), or cpl != 0: one head of 64 cpl columns
// narrow != 0 (option gat_fused_narrow): rows of 16 or 8 columns in the sweeps of gat_narrow.hip, S = 1
struct V2Route {
  int S, w, Hs, cpl, narrow;
};

// what both calls refuse before they touch anything: 0 = go on.  align_or: the fp32 buffers, and a table's part by table_align
// (gat_fused_seq.h: an fp32 table as it is, a bf16 table off an 8-byte boundary as a miss of the 16)
int gatv2_route(const char* who, gaib_ctx* ctx, gaib_graph* g, int len, int heads, uintptr_t align_or, V2Route* r) {
  *r = V2Route{1, len, heads, 0, 0};
  bool ok = gat_fused_shape(len, heads);
  if (!ok && ctx->gat_fused_narrow == 1 && gat_narrow_shape(len, heads)) r->narrow = 1, ok = true;
  if (!ok && ctx->gatv2_wide == 1) {
    int w = 0;
    const int S = gaib_gat_fused_slabs(len, heads, &w);
    if ((r->cpl = gaib_gat_fused_head_cpl(len, heads)) != 0) ok = true;
    else if (S >= 2) *r = V2Route{S, w, heads / S, 0, 0}, ok = true;
  }
  // (the sweeps' 32-bit byte offsets run over the caller's full rows: the bound is on nv * len, slabs or not, and on the fp32
  // form's bytes whatever the element type)
  if (!ok || g->nc != g->nv || (uint64_t)g->nv * (uint64_t)len * 4u >= ((uint64_t)1 << 32)) {
    gaib_set_error("%s: covers len 32, 64 or 128 with 1, 2, 4, 8 or 16 heads of at least 4 columns -- with option gatv2_wide = 1 also "
                   "column slabs of those shapes (gaib_gat_fused_slabs) and one head of 256 or 512 columns, with option gat_fused_narrow = 1 also "
                   "len 16 (1, 2 or 4 heads) and len 8 (1 or 2 heads) -- on a whole graph over tables below 4 GB (len %d, heads %d, %lld x %lld)", who, len, heads, (long long)g->nv, (long long)g->nc);
    return GAIB_ERR_UNSUPPORTED;
  }
  GAIB_CHECK((align_or & 15) == 0, "%s: buffers must be 16-byte aligned (bf16 tables: 8-byte)", who);
  return GAIB_OK;
}

// profile bytes of S sweeps at (w, Hs); the column ids and the chunks' partials once per slab.  A work rate in dense (fp32) bytes
// for both element types, as gat_bf16.hip reports the static-score sweeps
// forward: per edge the column id and one gathered row; per chunk the partial (acc, m, l) written and read; per row its own h, out and
// the statistics.  flops: per edge and column z, phi, the score's fma, and the accumulator's
double v2_bytes_fwd(const gaib_graph* g, int w, int Hs, int S) {
  return S * ((double)g->ne * (4.0 + 4.0 * w) + (double)g->n_chunks * (4.0 * w + 8.0 * Hs) * 2 + (double)g->nv * (2 * 4.0 * w + 8.0 * Hs));
}
// backward: per edge the column id, two gathered rows and the 12 bytes of a record per head; per chunk the partial row written and
// read; per row h, grad and the forward output read, grad_out written and 20 bytes per head of statistics and record; per workgroup
// its a-gradient partial written and read.  flops: per edge and column the score (5), two dots (4), the three accumulators (6).
// drop: the reverse-edge id, 4 more bytes per edge (the masks themselves move no byte)
double v2_bytes_bwd(const gaib_graph* g, int w, int Hs, int S, unsigned grid, bool drop) {
  return S * ((double)g->ne * ((drop ? 8.0 : 4.0) + 2 * 4.0 * w + 12.0 * Hs) + (double)g->n_chunks * 4.0 * w * 2 +
              (double)g->nv * (4 * 4.0 * w + 20.0 * Hs) + (double)grid * 4.0 * w * 2);
}

// Steps in flight: forward 8 for both element types (the v1 forward's; it fixes the order of the online softmax).  Backward 4 at
// every width and for both element types: three gathers per step; fp32 100 - 108 VGPRs, no spill, four waves per SIMD -- the
// 128-column instance needed no lower unroll.  On bf16 tables the raw rows of a batch wait in half the registers, but 8 steps in
// flight (no bit depends on the choice) took 114 - 136 VGPRs and left 43 of the 56 instances at three waves per SIMD: the widened
// copies and the per-step scalars of a longer batch outweigh the packed rows, as in gat_head.hip.  At 4 every bf16 instance is at
// or below its fp32 form (DESIGN 3.3.8 has the register table).
// Under DROP the unrolls stay: the one or two mask words did not cost a wave.
constexpr int V2_BWD_U = 4;

// One forward sweep and its row combine at (len, heads); WIDE: on windows of rows of ld elements and stats_ld records; DROP: under
// dw's masks (WIDE: its head window)
template <typename E, bool WIDE, bool DROP>
int v2_forward_sweep(gaib_ctx* ctx, const gaib_graph* g, int len, int heads, int ld, int stats_ld, const E* d_h, const float* d_a,
                     float eps, int relu, const FwdWs& ws, float* d_out, float* d_row_stats, const DropWin& dw) {
  unsigned grid;
  int per_xcd;
  chunk_grid(ctx, g, true, &grid, &per_xcd);
#define GAIB_V2_FWD(GG, HH)                                                                                                    \
  gatv2_fwd_chunk_kernel<GG, HH, 8, WIDE, DROP, E><<<grid, 256, 0, ctx->stream>>>(                                             \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, d_h, d_a, eps, ws.out_partial, ws.ms_partial, \
      per_xcd, ld, dw.rate, dw.scale, dw.seed, dw.mask_heads, dw.mask_head0)
  if (grid > 0) {
    GAIB_GAT_DISPATCH(GAIB_V2_FWD);
    GAIB_LAUNCH_CHECK();
  }
#undef GAIB_V2_FWD
  // (rows without an edge: zeros and statistics (-1e30, 0), as in v1)
#define GAIB_V2_FR(GG)                                                                                                              \
  gat_fwd_reduce_kernel<GG, WIDE><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, heads, g->chunk_start, ws.out_partial,      \
                                                                           ws.ms_partial, relu ? 1 : 0, d_out,                     \
                                                                           reinterpret_cast<float2*>(d_row_stats), ld, stats_ld)
  if (len == 32) GAIB_V2_FR(8);
  else if (len == 64) GAIB_V2_FR(16);
  else GAIB_V2_FR(32);
#undef GAIB_V2_FR
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// the backward's workspace at (w, Hs): records [nv][Hs] x 16 B | rowdot [nv][Hs] | partial rows [n_chunks][w] | a-gradient partials
// [grid][w] | their strips [nstrips][w]
// nparts: the partial vectors the two-level sum reads.  Undropped: one per workgroup, grid of them -- under option gat_chunk_xcd the
// walk changes which four chunks a workgroup holds, and with it the order of a's sum (the other outputs keep their bits).  The
// dropped sweeps store a workgroup's vector at the index of its four CHUNKS (blk, not blockIdx.x): vector b is the sum of chunks
// 4 b .. 4 b + 3 with or without the walk, the cdiv(n_chunks, 4) vectors that hold chunks are read and the strips follow from that
// count alone -- a's gradient has the same bits under gat_chunk_xcd = 1 (the walk's padding workgroups write zeros behind them,
// inside the [grid][w] the workspace holds).
struct V2BwdWs {
  f4* rec;
  float *rowdot, *out_partial, *ag_partial, *ag_strip;
  unsigned grid, nparts;
  int per_xcd, nstrips;
};
int v2_backward_ws(gaib_ctx* ctx, const gaib_graph* g, int w, int Hs, bool drop, V2BwdWs* ws) {
  chunk_grid(ctx, g, true, &ws->grid, &ws->per_xcd);
  const unsigned grid = ws->grid;
  const unsigned np = ws->nparts = drop ? (unsigned)cdiv64(g->n_chunks, 4) : grid;
  ws->nstrips = np == 0 ? 0 : (int)(np < 4096 ? cdiv64(np, 4) : 1024);
  const size_t n_v = up4((size_t)g->nv * Hs), n_op = up4((size_t)g->n_chunks * w);
  const size_t n_ag = (size_t)grid * w, n_st = (size_t)ws->nstrips * w;
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (5 * n_v + n_op + n_ag + n_st)));
  ws->rec = reinterpret_cast<f4*>(ctx->ws);
  ws->rowdot = (float*)ctx->ws + 4 * n_v;
  ws->out_partial = ws->rowdot + n_v;
  ws->ag_partial = ws->out_partial + n_op;
  ws->ag_strip = ws->ag_partial + n_ag;
  return GAIB_OK;
}

// a's gradient from the workgroups' partial vectors [nparts][len], two fixed levels
int v2_agrad(gaib_ctx* ctx, const V2BwdWs& ws, int len, float* d_a_grad) {
  if (ws.nparts > 0) {
    gatv2_agrad_strip_kernel<<<ws.nstrips, 256, 0, ctx->stream>>>((int64_t)ws.nparts, len, ws.ag_partial,
                                                                  cdiv64(ws.nparts, ws.nstrips), ws.ag_strip);
    GAIB_LAUNCH_CHECK();
  }
  gatv2_agrad_final_kernel<<<(unsigned)cdiv64(len, 4), 256, 0, ctx->stream>>>(ws.nstrips, len, ws.ag_strip, d_a_grad);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// one backward sweep with its prologue and reductions at (len, heads); WIDE: on windows of rows of ld elements and stats_ld records
// DROP: under dw's masks; the sweep reads g->rev
template <typename E, bool WIDE, bool DROP>
int v2_backward_sweep(gaib_ctx* ctx, const gaib_graph* g, int len, int heads, int ld, int stats_ld, const E* d_feat, const E* d_grad,
                      const float* d_fwd_out, const float* d_a, const float* d_row_stats, float eps, const V2BwdWs& ws,
                      float* d_grad_out, float* d_a_grad, const DropWin& dw) {
  GAIB_TRY((gat_bwd_prologue<E, WIDE>(ctx, g->nv, len, heads, ld, stats_ld, d_grad, d_fwd_out, d_row_stats, ws.rowdot, ws.rec)));
  const unsigned grid = ws.grid;
  const int per_xcd = ws.per_xcd;
#define GAIB_V2_BWD(GG, HH)                                                                                                     \
  gatv2_bwd_chunk_kernel<GG, HH, V2_BWD_U, WIDE, DROP, E><<<grid, 256, 0, ctx->stream>>>(                                       \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, d_feat, d_grad, ws.rec, d_a, eps,         \
      ws.out_partial, ws.ag_partial, per_xcd, ld, g->rev, dw.rate, dw.scale, dw.seed, dw.mask_heads, dw.mask_head0)
  if (grid > 0) {
    GAIB_GAT_DISPATCH(GAIB_V2_BWD);
    GAIB_LAUNCH_CHECK();
  }
#undef GAIB_V2_BWD
  GAIB_TRY(v2_agrad(ctx, ws, len, d_a_grad));
  // the rows' partial sums in chunk order (H = 0: the kernel's row / column sums of v1 have no part here, nothing of them is read
  // or written)
#define GAIB_V2_RD(GG)                                                                                                               \
  gat_fused_reduce_kernel<GG, WIDE><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, len, 0, g->chunk_start, ws.out_partial, nullptr, \
                                                                             d_grad_out, nullptr, nullptr, ld)
  if (len == 32) GAIB_V2_RD(8);
  else if (len == 64) GAIB_V2_RD(16);
  else GAIB_V2_RD(32);
#undef GAIB_V2_RD
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// what a dropped call checks ahead of the route: the rate
int v2_check_drop(const char* who, const DropWin* drop) {
  if (drop) GAIB_CHECK(drop->rate >= 0.f && drop->rate < 1.f, "%s: rate must be in [0,1)", who);
  return GAIB_OK;
}

// the forward call; drop: NULL, or rate, scale and seed of the _drop call (the window fields are set here, per slab)
template <typename E>
int v2_forward_seq(const char* who, gaib_ctx* ctx, gaib_graph* g, int len, int heads, const E* d_h, const float* d_a, float eps,
                   int relu, float* d_out, float* d_row_stats, const DropWin* drop) {
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_TRY(check_heads(who, len, heads));
  GAIB_TRY(v2_check_drop(who, drop));
  V2Route r;
  GAIB_TRY(gatv2_route(who, ctx, g, len, heads, table_align(d_h) | (uintptr_t)d_a | (uintptr_t)d_out | (uintptr_t)d_row_stats, &r));
  if (g->nv == 0) return GAIB_OK;
  GAIB_CHECK(d_h && d_a && d_out && d_row_stats && (const void*)d_out != (const void*)d_h, "%s: NULL or aliased pointer", who);
  GAIB_HIP(hipSetDevice(ctx->device));
  if (drop) GAIB_TRY(gaib_graph_ensure_rev(ctx, g));  // (not read here: forward and backward must decide alike)
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  FwdWs ws;
  GAIB_TRY(gat_forward_ws(ctx, g, r.w, r.Hs, &ws));
  ProfScope ps(ctx, "gatv2_fwd", v2_bytes_fwd(g, r.w, r.Hs, r.S), 7.0 * (double)g->ne * len);
  if (r.cpl) {
    unsigned grid;
    int per_xcd;
    chunk_grid(ctx, g, true, &grid, &per_xcd);
    return gatv2_head_forward_run<E>(ctx, g, r.cpl, grid, per_xcd, d_h, d_a, eps, relu, ws.out_partial, ws.ms_partial, d_out,
                                     d_row_stats, drop);
  }
  DropWin dw = drop ? *drop : DropWin{0.f, 1.f, 0, 0, 0};
  dw.mask_heads = heads;
  if (r.narrow) {
    unsigned grid;
    int per_xcd;
    chunk_grid(ctx, g, true, &grid, &per_xcd);
    dw.mask_head0 = 0;
    return gatv2_narrow_forward_run<E>(ctx, g, len, heads, grid, per_xcd, d_h, d_a, eps, relu, ws.out_partial,
                                       reinterpret_cast<float*>(ws.ms_partial), d_out, d_row_stats, drop ? &dw : nullptr);
  }
  if (r.S == 1) {
    dw.mask_head0 = 0;
    return drop ? v2_forward_sweep<E, false, true>(ctx, g, len, heads, len, heads, d_h, d_a, eps, relu, ws, d_out, d_row_stats, dw)
                : v2_forward_sweep<E, false, false>(ctx, g, len, heads, len, heads, d_h, d_a, eps, relu, ws, d_out, d_row_stats, dw);
  }
  for (int s = 0; s < r.S; ++s) {
    const int c = s * r.w;
    dw.mask_head0 = s * r.Hs;  // slab s reads the masks of ITS heads in the full row's [ne][heads] array
    float* st = d_row_stats + 2 * s * r.Hs;
    GAIB_TRY(drop ? (v2_forward_sweep<E, true, true>(ctx, g, r.w, r.Hs, len, heads, d_h + c, d_a + c, eps, relu, ws, d_out + c, st, dw))
                  : (v2_forward_sweep<E, true, false>(ctx, g, r.w, r.Hs, len, heads, d_h + c, d_a + c, eps, relu, ws, d_out + c, st, dw)));
  }
  return GAIB_OK;
}

// the backward call; drop as in v2_forward_seq
template <typename E>
int v2_backward_seq(const char* who, gaib_ctx* ctx, gaib_graph* g, int len, int heads, const E* d_feat, const E* d_grad,
                    const float* d_fwd_out, const float* d_a, const float* d_row_stats, float eps, float* d_grad_out, float* d_a_grad,
                    const DropWin* drop) {
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_TRY(check_heads(who, len, heads));
  GAIB_TRY(v2_check_drop(who, drop));
  V2Route r;
  GAIB_TRY(gatv2_route(who, ctx, g, len, heads,
                       table_align(d_feat) | table_align(d_grad) | (uintptr_t)d_fwd_out | (uintptr_t)d_a | (uintptr_t)d_row_stats |
                           (uintptr_t)d_grad_out | (uintptr_t)d_a_grad,
                       &r));
  GAIB_CHECK(d_a_grad, "%s: NULL pointer", who);
  if (g->nv == 0) return zero_alpha_grads(ctx, len, d_a_grad, nullptr);
  GAIB_CHECK(d_feat && d_grad && d_fwd_out && d_a && d_row_stats && d_grad_out, "%s: NULL pointer", who);
  GAIB_CHECK((const void*)d_grad_out != (const void*)d_feat && (const void*)d_grad_out != (const void*)d_grad && d_grad_out != d_fwd_out,
             "%s: d_grad_out must not alias an input", who);
  GAIB_HIP(hipSetDevice(ctx->device));
  // the single sweep takes the in-edges of a row for the reverses of its own edges: a graph that is not structurally symmetric is
  // an error, the permutation's own (the undropped sweep does not read it; the dropped one takes the reverse edges' masks from it)
  GAIB_TRY(gaib_graph_ensure_rev(ctx, g));
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  V2BwdWs ws;
  GAIB_TRY(v2_backward_ws(ctx, g, r.w, r.Hs, drop != nullptr, &ws));
  ProfScope ps(ctx, "gatv2_bwd", v2_bytes_bwd(g, r.w, r.Hs, r.S, ws.grid, drop != nullptr), 15.0 * (double)g->ne * len);
  if (r.cpl) {
    GAIB_TRY((gat_bwd_prologue<E, false>(ctx, g->nv, len, 1, len, 1, d_grad, d_fwd_out, d_row_stats, ws.rowdot, ws.rec)));
    GAIB_TRY(gatv2_head_backward_run<E>(ctx, g, r.cpl, ws.grid, ws.per_xcd, d_feat, d_grad, ws.rec, d_a, eps, ws.out_partial,
                                        ws.ag_partial, d_grad_out, drop));
    return v2_agrad(ctx, ws, len, d_a_grad);
  }
  DropWin dw = drop ? *drop : DropWin{0.f, 1.f, 0, 0, 0};
  dw.mask_heads = heads;
  if (r.narrow) {
    dw.mask_head0 = 0;
    GAIB_TRY((gat_bwd_prologue<E, false>(ctx, g->nv, len, heads, len, heads, d_grad, d_fwd_out, d_row_stats, ws.rowdot, ws.rec)));
    GAIB_TRY(gatv2_narrow_backward_run<E>(ctx, g, len, heads, ws.grid, ws.per_xcd, d_feat, d_grad, reinterpret_cast<const float*>(ws.rec),
                                          d_a, eps, ws.out_partial, ws.ag_partial, d_grad_out, drop ? &dw : nullptr));
    return v2_agrad(ctx, ws, len, d_a_grad);
  }
  if (r.S == 1) {
    dw.mask_head0 = 0;
    return drop ? v2_backward_sweep<E, false, true>(ctx, g, len, heads, len, heads, d_feat, d_grad, d_fwd_out, d_a, d_row_stats, eps, ws,
                                                    d_grad_out, d_a_grad, dw)
                : v2_backward_sweep<E, false, false>(ctx, g, len, heads, len, heads, d_feat, d_grad, d_fwd_out, d_a, d_row_stats, eps,
                                                     ws, d_grad_out, d_a_grad, dw);
  }
  for (int s = 0; s < r.S; ++s) {
    const int c = s * r.w;
    dw.mask_head0 = s * r.Hs;
    const float* st = d_row_stats + 2 * s * r.Hs;
    GAIB_TRY(drop ? (v2_backward_sweep<E, true, true>(ctx, g, r.w, r.Hs, len, heads, d_feat + c, d_grad + c, d_fwd_out + c, d_a + c, st,
                                                      eps, ws, d_grad_out + c, d_a_grad + c, dw))
                  : (v2_backward_sweep<E, true, false>(ctx, g, r.w, r.Hs, len, heads, d_feat + c, d_grad + c, d_fwd_out + c, d_a + c, st,
                                                       eps, ws, d_grad_out + c, d_a_grad + c, dw)));
  }
  return GAIB_OK;
}

}  // namespace
