// gat_fused_seq.h -- the host side of the one-sweep GAT, once: argument checks, workspace layouts, profile formulas and the launch
// sequences of every public one-sweep call, templated on the element type E of the gathered tables (float: gat_fused.hip;
// uint16_t = raw bf16 bits: gat_bf16.hip).  Only the tables (h; feat and grad) have the type E; records, statistics, alpha
// vectors, partial sums and every output are fp32.
//
//   forward:   workspace, chunk grid (+ XCD walk), chunk sweep, gat_fwd_reduce_kernel
//   backward:  workspace, rowdot_kernel, records, chunk sweep, gat_fused_reduce_kernel, alpha_partial_kernel, alpha_final_kernel
//
// A call is the sequence over S column slabs of w columns and Hs = heads / S heads: S = 1 (w = len) at the shapes the kernels cover,
// S >= 2 with option gat_fused_wide on a multi-head row wider than 128 columns (gaib_gat_fused_slabs).  Heads are independent in
// everything the sweeps compute, and the chunk list, the order of a chunk's steps, the chunk-order reductions and the block
// partition of the alpha reductions follow from the graph and nv alone: every slab's outputs have the BITS of the narrow call at
// (w, Hs) on contiguous copies of its column windows.  What a slab keeps to itself lives in the workspace at the slab's own width
// and is reused by the next slab (same stream); only the caller's arrays are strided ([nv][len] tables, d_row_stats [nv][heads][2]).
// Under attention dropout the mask of (edge e, head k of slab s) is the full row's: element e heads + s Hs + k of the virtual
// [ne][heads] mask array, reached through a head window (DropWin; gat_drop_bits<.., WIN>).
//
// THE INSTANTIATION EACH CALL REACHES (template arguments of gat_fwd_fused_chunk_kernel<G, H, 8, E, DROP, WIDE> and
// gat_bwd_fused_chunk_kernel<G, H, U, RECOMP, E, DROP, WIN>; U = 8 only for G == 16 with gat_fused_unroll == 8, else 4):
//
//   call                                  | forward sweep            | backward sweep
//   --------------------------------------+--------------------------+----------------------------------------------------------
//   fused fp32, narrow                    | <G,H,8,float>            | <G,H,U,RECOMP,float>, RECOMP = (d_row_stats != NULL);
//                                         |                          |   gat_interleave = 1: the same on the interleaved table;
//                                         |                          |   gat_bwd_pk = 1: gat_bwd_fused_pk_kernel<G,H,4,float>
//   fused fp32 _rect                      | <G,H,8,float> + phase    | <G,H,4,true,float> + phase, rec_ld = H, no XCD walk
//   _drop fp32, narrow                    | <G,H,8,float,true>       | <G,H,U,true,float,true>
//   _bf16, narrow                         | <G,H,8,uint16_t>         | <G,H,U,true,uint16_t>;
//                                         |                          |   gat_bwd_pk = 1: gat_bwd_fused_pk_kernel<G,H,4,uint16_t>
//   _drop_win fp32; _drop_bf16, narrow    | <G,H,8,E,true,true>      | <G,H,U,true,E,true,true>
//   any, wide, undropped                  | <G,H,8,E,false,true>/slab| <G,H,U,true,E> with ld = len
//   any, wide, dropped                    | <G,H,8,E,true,true>/slab | <G,H,U,true,E,true,true>
//
// The narrow _drop_bf16 call is the WINDOW form with ld = len and the window (heads, 0) ON PURPOSE: it is what a dropped bf16 slab
// runs, so bf16 tables have no <.., DROP> instantiation without WIDE / WIN, where fp32 keeps its own narrow _drop form.  Whether
// the narrow fp32 calls could run the strided forms too is a speed question with its own measurement; nothing here decides it.
// The helper kernels follow `strided` (slab and window calls): the WIDE rowdot, records, reduce and alpha_partial kernels there,
// the plain ones in the narrow calls.  gat_bwd_pk and gat_interleave are read by the narrow undropped row-statistics calls only.
#pragma once
#include <type_traits>

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

// attention dropout: rate, scale and seed of the call, and the sweep's window into the [ne][mask_heads] mask array
struct DropWin {
  float rate, scale;
  uint64_t seed;
  int mask_heads, mask_head0;
};

// the public calls' arguments, and -- with (len, heads) = (w, Hs), the pointers at the slab's first column / head -- one slab's.
// ld / stats_ld: row strides of the caller's tables and of d_row_stats (float2 records); strided: the WIDE / WIN kernel forms.
template <typename E>
struct GatFwd {
  const char* who;
  int len, heads;
  const E* h;
  const float *alpha_l, *alpha_r;
  float eps;
  int relu;
  float *out, *row_stats;
  const DropWin* drop = nullptr;  // NULL: no attention dropout
  bool win = false;               // the caller names the mask window (gaib_gat_*_fused_drop_win)
  int phase = -1;
  bool rect = false;
  int ld = 0, stats_ld = 0;
  bool strided = false;
};
template <typename E>
struct GatBwd {
  const char* who;
  int len, heads;
  const E *feat, *grad;
  const float *fwd_out, *alpha_l, *alpha_r;
  const float *norm_scores, *row_stats;  // the attention array (fp32 undropped only), or the forward's statistics: RECOMP
  const float* rec_tab;                  // _rect: the records of every column vertex, made by the caller
  float eps;
  float *grad_out, *alpha_lgrad, *alpha_rgrad;
  const DropWin* drop = nullptr;
  bool win = false;
  int phase = -1;
  bool rect = false;
  int ld = 0, stats_ld = 0, rec_ld = 0;
  bool strided = false, unroll8 = false;
  const f4* rec = nullptr;
};

int gat_refuse(const char* who, int len, int heads) {
  gaib_set_error("%s: not applicable to this shape / graph (len %d, heads %d)", who, len, heads);
  return GAIB_ERR_UNSUPPORTED;
}

// a table's part in the 16-byte alignment test of the fp32 buffers: an fp32 table as it is; a bf16 table must be 8-byte aligned
// (a lane's four columns are one 8-byte load), reported as a miss of the 16
uintptr_t table_align(const float* p) { return (uintptr_t)p; }
uintptr_t table_align(const uint16_t* p) { return ((uintptr_t)p & 7) ? 15 : 0; }

// what every call checks before it looks at the graph or the device
int gat_check_call(const char* who, const gaib_ctx* ctx, const gaib_graph* g, int len, int heads, int phase, const DropWin* drop,
                   bool win) {
  GAIB_CHECK(ctx && g, "%s: NULL ctx/graph", who);
  GAIB_TRY(check_heads(who, len, heads));
  GAIB_CHECK(phase >= -1 && phase <= 1, "%s: phase is -1, 0 or 1", who);
  if (drop) GAIB_CHECK(drop->rate >= 0.f && drop->rate < 1.f, "%s: rate must be in [0,1)", who);
  if (win)
    GAIB_CHECK(drop->mask_head0 >= 0 && (int64_t)drop->mask_head0 + heads <= (int64_t)drop->mask_heads,
               "%s: heads [%d, %d + %d) are no window of %d mask heads", who, drop->mask_head0, drop->mask_head0, heads, drop->mask_heads);
  return GAIB_OK;
}
template <typename E>
int gat_check_ptrs(const GatFwd<E>& a) {
  GAIB_CHECK(a.h && a.alpha_l && a.alpha_r && a.out && a.row_stats && (const void*)a.out != (const void*)a.h,
             "%s: NULL or aliased pointer", a.who);
  return GAIB_OK;
}
template <typename E>
int gat_check_ptrs(const GatBwd<E>& a) {
  if (a.drop || !std::is_same<E, float>::value)
    GAIB_CHECK(a.row_stats, "%s: d_row_stats is NULL (only gaib_gat_backward_fused has an attention-array form)", a.who);
  GAIB_CHECK(a.feat && a.grad && a.alpha_l && a.alpha_r && a.grad_out && a.alpha_lgrad && a.alpha_rgrad &&
                 (a.rect ? a.rec_tab != nullptr : a.fwd_out && (a.norm_scores || a.row_stats)),
             "%s: NULL pointer", a.who);
  GAIB_CHECK((const void*)a.grad_out != (const void*)a.feat && (const void*)a.grad_out != (const void*)a.grad,
             "%s: d_grad_out must not alias an input", a.who);
  return GAIB_OK;
}

// no rows: the alpha gradients of this graph are zero, nothing else is written
int zero_alpha_grads(gaib_ctx* ctx, int len, float* d_alpha_lgrad, float* d_alpha_rgrad) {
  GAIB_HIP(hipSetDevice(ctx->device));
  if (d_alpha_lgrad) GAIB_HIP(hipMemsetAsync(d_alpha_lgrad, 0, sizeof(float) * len, ctx->stream));
  if (d_alpha_rgrad) GAIB_HIP(hipMemsetAsync(d_alpha_rgrad, 0, sizeof(float) * len, ctx->stream));
  return GAIB_OK;
}

// option gat_fused_wide: the number of column slabs S >= 2 of a multi-head row wider than 128 columns, *w their width; else 1, len
int gat_wide_route(const gaib_ctx* ctx, int len, int heads, int* w) {
  *w = len;
  if (ctx->gat_fused_wide != 1 || gat_fused_shape(len, heads)) return 1;
  int ws = 0;
  const int S = gaib_gat_fused_slabs(len, heads, &ws);
  if (S < 2) return 1;
  *w = ws;
  return S;
}

// four chunks per workgroup (0 on a rank whose rows have no edges: nothing to sweep); option gat_chunk_xcd: see the kernels' per_xcd
void chunk_grid(const gaib_ctx* ctx, const gaib_graph* g, bool xcd_walk, unsigned* grid, int* per_xcd) {
  *grid = (unsigned)cdiv64(g->n_chunks, 4);
  *per_xcd = 0;
  if (xcd_walk && ctx->gat_chunk_xcd == 1 && *grid >= 64) {
    *per_xcd = (int)cdiv64(*grid, 8);
    *grid = (unsigned)*per_xcd * 8u;
  }
}

// profile bytes of S sweeps at (w, Hs): the column ids and the chunk headers are read once per slab.  The fp32 formula on bf16
// tables and under dropout too: the achieved rate is a work rate in dense bytes, and the mask moves no byte.
double gat_prof_bytes_fwd(const gaib_graph* g, int w, int Hs, int S) {
  return S * ((double)g->ne * (4.0 + 4.0 * w) + (double)g->n_chunks * (4.0 * w + 8.0 * Hs) * 2 + (double)g->nv * (4.0 * w + 8.0 * Hs));
}
double gat_prof_bytes_bwd(const gaib_graph* g, int w, int Hs, int S) {
  return S * ((double)g->ne * (4.0 + 2 * 4.0 * w + 12.0 * Hs) + (double)g->n_chunks * (4.0 * w + 8.0 * Hs) * 2 + (double)g->nv * 3 * 4.0 * w);
}

// ---- workspace at the width (w, Hs) of one sweep -------------------------------------------------------------------------------------
struct FwdWs {
  float* out_partial;  // [n_chunks][w]
  float2* ms_partial;  // [n_chunks][Hs]
};
int gat_forward_ws(gaib_ctx* ctx, const gaib_graph* g, int w, int Hs, FwdWs* ws) {
  const size_t n_op = up4((size_t)g->n_chunks * w), n_ms = up4((size_t)g->n_chunks * Hs * 2);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (n_op + n_ms)));
  ws->out_partial = (float*)ctx->ws;
  ws->ms_partial = reinterpret_cast<float2*>(ws->out_partial + n_op);
  return GAIB_OK;
}

// records: rec and rowdot are made here (not in _rect, whose caller brings the records: its phase-0 and phase-1 calls see the same
// layout, the partials live here between the two).  table_floats: the interleaved or packed table, on its 256-byte boundary.
struct BwdWs {
  f4* rec;  // [nv][Hs] 16-byte records (first: alignment)
  float *rowdot, *rs, *cs, *out_partial, *rc_partial, *partial;
  void* table;
};
int gat_backward_ws(gaib_ctx* ctx, const gaib_graph* g, int w, int Hs, bool records, size_t table_floats, BwdWs* ws) {
  const size_t n_ap = (size_t)gat_alpha_blocks(g->nv) * 2 * w;  // the alpha gradients' block partials
  const size_t n_v = up4((size_t)g->nv * Hs);
  const size_t n_op = up4((size_t)g->n_chunks * w), n_rc = up4((size_t)g->n_chunks * 2 * Hs);
  const size_t n_t = table_floats ? table_floats + 64 : 0;  // (+ 64 floats: the table starts on a 256-B boundary)
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * ((records ? 7 : 2) * n_v + n_op + n_rc + n_ap + n_t)));
  float* p = (float*)ctx->ws;
  ws->rec = records ? reinterpret_cast<f4*>(p) : nullptr;
  ws->rowdot = records ? p + 4 * n_v : nullptr;
  ws->rs = records ? p + 5 * n_v : p;
  ws->cs = ws->rs + n_v;
  ws->out_partial = ws->cs + n_v;
  ws->rc_partial = ws->out_partial + n_op;
  ws->partial = ws->rc_partial + n_rc;
  ws->table = reinterpret_cast<void*>(((uintptr_t)(ws->partial + n_ap) + 255) & ~(uintptr_t)255);
  return GAIB_OK;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
template <typename E, bool DROP, bool WIDE>
void gat_fwd_sweep_launch(gaib_ctx* ctx, const gaib_graph* g, const GatFwd<E>& q, const FwdWs& ws, unsigned grid, int per_xcd) {
  const int len = q.len, heads = q.heads;
  const DropWin dw = q.drop ? *q.drop : DropWin{0.f, 1.f, 0, 0, 0};
#define GAIB_FF(GG, HH)                                                                                                        \
  gat_fwd_fused_chunk_kernel<GG, HH, 8, E, DROP, WIDE><<<grid, 256, 0, ctx->stream>>>(                                         \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, len, q.h, q.alpha_l, q.alpha_r, q.eps,   \
      ws.out_partial, ws.ms_partial, q.phase, (uint32_t)g->nv, per_xcd, dw.rate, dw.scale, dw.seed, q.ld, dw.mask_heads,       \
      dw.mask_head0)
  GAIB_GAT_DISPATCH(GAIB_FF);
#undef GAIB_FF
}

// the chunk sweep of one slab; the instantiation follows the table above
template <typename E>
int gat_fwd_sweep(gaib_ctx* ctx, const gaib_graph* g, const GatFwd<E>& q, const FwdWs& ws) {
  unsigned grid;
  int per_xcd;
  chunk_grid(ctx, g, !q.rect, &grid, &per_xcd);
  if (grid == 0) return GAIB_OK;
  if (q.drop && q.strided) gat_fwd_sweep_launch<E, true, true>(ctx, g, q, ws, grid, per_xcd);
  else if (q.strided) gat_fwd_sweep_launch<E, false, true>(ctx, g, q, ws, grid, per_xcd);
  else if (!q.drop) gat_fwd_sweep_launch<E, false, false>(ctx, g, q, ws, grid, per_xcd);
  else if constexpr (std::is_same<E, float>::value) gat_fwd_sweep_launch<E, true, false>(ctx, g, q, ws, grid, per_xcd);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

template <typename E, bool WIDE>
int gat_fwd_reduce(gaib_ctx* ctx, const gaib_graph* g, const GatFwd<E>& q, const FwdWs& ws) {
#define GAIB_FR(GG)                                                                                                          \
  gat_fwd_reduce_kernel<GG, WIDE><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, q.len, q.heads, g->chunk_start, ws.out_partial, \
                                                                           ws.ms_partial, q.relu ? 1 : 0, q.out,              \
                                                                           reinterpret_cast<float2*>(q.row_stats), q.ld, q.stats_ld)
  if (q.len == 32) GAIB_FR(8);
  else if (q.len == 64) GAIB_FR(16);
  else GAIB_FR(32);
#undef GAIB_FR
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// a public forward call: a.len / a.heads are the full row's
template <typename E>
int gat_forward_fused_seq(gaib_ctx* ctx, gaib_graph* g, GatFwd<E> a) {
  const char* who = a.who;
  const int len = a.len, heads = a.heads;
  GAIB_TRY(gat_check_call(who, ctx, g, len, heads, a.phase, a.drop, a.win));
  if (g->nv == 0 || (a.drop && g->nc != g->nv)) {
    // a rank without rows (fewer vertices than ranks): nothing to write, its buffers may be NULL -- but WHICH path "ran" must be
    // what the ranks with rows decide, from the shape and the option alone: the two paths differ in their exchanges
    if (a.rect && gat_fused_shape(len, heads) && ctx->gat_fused_fwd != 0) return GAIB_OK;
    return gat_refuse(who, len, heads);  // (the dropped calls have no _rect form)
  }
  GAIB_TRY(gat_check_ptrs(a));
  GAIB_HIP(hipSetDevice(ctx->device));
  int w = len, rc = GAIB_OK;
  const int S = (a.rect || a.win) ? 1 : gat_wide_route(ctx, len, heads, &w);  // whole graphs only: _rect keeps its answer
  const int Hs = heads / S;
  const uintptr_t align_or = table_align(a.h) | (uintptr_t)a.out | (uintptr_t)a.row_stats | (uintptr_t)a.alpha_l | (uintptr_t)a.alpha_r;
  if (!gat_fused_applies(ctx, g, w, Hs, ctx->gat_fused_fwd, align_or, &rc, a.rect)) return rc != GAIB_OK ? rc : gat_refuse(who, len, heads);
  if (a.drop) GAIB_TRY(gaib_graph_ensure_rev(ctx, g));  // (not read here: forward and backward must decide alike)
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  FwdWs ws;
  GAIB_TRY(gat_forward_ws(ctx, g, w, Hs, &ws));
  ProfScope ps(ctx, "gat_fwd_fused", gat_prof_bytes_fwd(g, w, Hs, S), 4.0 * (double)g->ne * len);
  a.strided = S >= 2 || a.win || (a.drop && !std::is_same<E, float>::value);
  a.len = w, a.heads = Hs, a.ld = len, a.stats_ld = heads;
  for (int s = 0; s < S; ++s) {
    GatFwd<E> q = a;
    DropWin dw = {};
    if (a.drop) dw = *a.drop, dw.mask_head0 += s * Hs, q.drop = &dw;
    q.h += s * w, q.alpha_l += s * w, q.alpha_r += s * w, q.out += s * w, q.row_stats += 2 * s * Hs;
    GAIB_TRY(gat_fwd_sweep(ctx, g, q, ws));
    if (q.phase == 0) return GAIB_OK;  // the partial results live in the workspace until phase 1: no other call in between
    GAIB_TRY(q.strided ? (gat_fwd_reduce<E, true>(ctx, g, q, ws)) : (gat_fwd_reduce<E, false>(ctx, g, q, ws)));
  }
  return GAIB_OK;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// rowdot[v][h] = <grad_v, out_v>_h, then the records rec[v][h] = (rowdot, row maximum, 1 / row sum, 0) where the statistics exist
template <typename E, bool WIDE>
int gat_bwd_prologue(gaib_ctx* ctx, int64_t nv, int len, int heads, int ld, int stats_ld, const E* d_grad, const float* d_fwd_out,
                     const float* d_row_stats, float* rowdot, f4* rec) {
  rowdot_kernel<E, WIDE><<<rowgrid(nv), 256, 0, ctx->stream>>>(nv, len, heads, d_grad, d_fwd_out, rowdot, ld);
  GAIB_LAUNCH_CHECK();
  if (!d_row_stats) return GAIB_OK;
  const int64_t nrec = nv * (int64_t)heads;
  const unsigned grid = (unsigned)cdiv64(nrec, 256);
  const float2* stats = reinterpret_cast<const float2*>(d_row_stats);
  if (WIDE) gat_rec_wide_kernel<<<grid, 256, 0, ctx->stream>>>(nrec, heads, stats_ld, rowdot, stats, rec);
  else gat_rec_kernel<<<grid, 256, 0, ctx->stream>>>(nrec, rowdot, stats, rec);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

template <typename E, bool RECOMP, bool DROP, bool WIN>
void gat_bwd_sweep_launch(gaib_ctx* ctx, const gaib_graph* g, const GatBwd<E>& q, const BwdWs& ws, unsigned grid, int per_xcd) {
  const int len = q.len, heads = q.heads;
  const DropWin dw = q.drop ? *q.drop : DropWin{0.f, 1.f, 0, 0, 0};
  // the chunk kernel takes its row strides as they are (ld, rec_ld); rev is read by the attention-array and the dropped forms
#define GAIB_FB_U(GG, HH, UU)                                                                                                    \
  gat_bwd_fused_chunk_kernel<GG, HH, UU, RECOMP, E, DROP, WIN><<<grid, 256, 0, ctx->stream>>>(                                    \
      g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, g->rev, len, q.feat, q.grad, q.norm_scores, \
      nullptr, ws.rowdot, q.alpha_l, q.alpha_r, q.eps, ws.out_partial, ws.rc_partial, q.rec, q.phase, (uint32_t)g->nv, q.ld,      \
      q.rec_ld, per_xcd, dw.rate, dw.scale, dw.seed, dw.mask_heads, dw.mask_head0)
  // (8 edges in flight per group is an option of the 64-wide form only, where it was measured)
#define GAIB_FB(GG, HH)                              \
  do {                                               \
    if (GG == 16 && q.unroll8) GAIB_FB_U(16, HH, 8); \
    else GAIB_FB_U(GG, HH, 4);                       \
  } while (0)
  GAIB_GAT_DISPATCH(GAIB_FB);
#undef GAIB_FB
#undef GAIB_FB_U
}

// the chunk sweep over q's tables and records; the instantiation follows the table above
template <typename E>
int gat_bwd_sweep(gaib_ctx* ctx, const gaib_graph* g, const GatBwd<E>& q, const BwdWs& ws, unsigned grid, int per_xcd) {
  if (grid == 0) return GAIB_OK;
  if (q.drop && q.strided) gat_bwd_sweep_launch<E, true, true, true>(ctx, g, q, ws, grid, per_xcd);
  else if (!q.drop && (q.row_stats || q.rect)) gat_bwd_sweep_launch<E, true, false, false>(ctx, g, q, ws, grid, per_xcd);
  else if constexpr (std::is_same<E, float>::value) {
    if (q.drop) gat_bwd_sweep_launch<E, true, true, false>(ctx, g, q, ws, grid, per_xcd);
    else gat_bwd_sweep_launch<E, false, false, false>(ctx, g, q, ws, grid, per_xcd);
  }
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// option gat_interleave (fp32): the three per-vertex tables of the sweep as one [h | grad | records] row per vertex
template <typename E>
int gat_bwd_sweep_interleaved(gaib_ctx* ctx, const gaib_graph* g, const GatBwd<E>& q, const BwdWs& ws, unsigned grid, int per_xcd) {
  const int len = q.len, ldt = 2 * len + 4 * q.heads;
  float* T = static_cast<float*>(ws.table);
  const int64_t tot4 = g->nv * (int64_t)(ldt / 4);
  gat_interleave_kernel<<<(unsigned)std::min<int64_t>(cdiv64(tot4, 256), (int64_t)ctx->num_cus * 16), 256, 0, ctx->stream>>>(
      g->nv, len / 4, q.heads, reinterpret_cast<const f4*>(q.feat), reinterpret_cast<const f4*>(q.grad), ws.rec, reinterpret_cast<f4*>(T));
  GAIB_LAUNCH_CHECK();
  GatBwd<E> t = q;
  t.feat = T, t.grad = T + len, t.rec = reinterpret_cast<const f4*>(T + 2 * len), t.ld = ldt, t.rec_ld = ldt / 4;
  return gat_bwd_sweep(ctx, g, t, ws, grid, per_xcd);
}

// option gat_bwd_pk: the packed-math sweep (gat_bwd_fused_pk_kernel) over a table whose rows pair h and grad element by element,
// then the fp32 records.  fp32 tables: 2 len + 4 heads dwords per vertex; bf16: len (h_k low half, g_k high half) + 4 heads.
template <typename E>
int gat_packed_row(int len, int heads) {
  return (std::is_same<E, float>::value ? 2 : 1) * len + 4 * heads;
}
template <typename E>
int gat_bwd_sweep_packed(gaib_ctx* ctx, const gaib_graph* g, const GatBwd<E>& q, const BwdWs& ws, unsigned grid, int per_xcd) {
  const int len = q.len, heads = q.heads;
  const int64_t tot4 = g->nv * (int64_t)(gat_packed_row<E>(len, heads) / 4);
  const unsigned pgrid = (unsigned)std::min<int64_t>(cdiv64(tot4, 256), (int64_t)ctx->num_cus * 16);
  if constexpr (std::is_same<E, float>::value)
    gat_interleave_pairs_kernel<<<pgrid, 256, 0, ctx->stream>>>(g->nv, len / 4, heads, reinterpret_cast<const f4*>(q.feat),
                                                                reinterpret_cast<const f4*>(q.grad), ws.rec, static_cast<f4*>(ws.table));
  else
    gat_pairs_bf16_kernel<<<pgrid, 256, 0, ctx->stream>>>(g->nv, len / 4, heads, reinterpret_cast<const u32x2*>(q.feat),
                                                          reinterpret_cast<const u32x2*>(q.grad), ws.rec, static_cast<u32x4*>(ws.table));
  GAIB_LAUNCH_CHECK();
#define GAIB_FBP(GG, HH)                                                                                                        \
  launch_bwd_pk<GG, HH, E>(grid, ctx->stream, g->n_chunks, g->chunk_row, g->chunk_ebase, g->chunk_start, g->rowptr, g->colidx, len, \
                           static_cast<const E*>(ws.table), q.alpha_l, q.alpha_r, q.eps, ws.out_partial, ws.rc_partial, per_xcd)
  GAIB_GAT_DISPATCH(GAIB_FBP);
#undef GAIB_FBP
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// the rows' sums in chunk order -> grad_out, rs, cs; then the alpha gradients over the rows (fixed two-level reduction)
template <typename E, bool WIDE>
int gat_bwd_epilogue(gaib_ctx* ctx, const gaib_graph* g, const GatBwd<E>& q, const BwdWs& ws) {
#define GAIB_FRD(GG)                                                                                                            \
  gat_fused_reduce_kernel<GG, WIDE><<<rowgrid(g->nv), 256, 0, ctx->stream>>>(g->nv, q.len, q.heads, g->chunk_start, ws.out_partial, \
                                                                             ws.rc_partial, q.grad_out, ws.rs, ws.cs, q.ld)
  if (q.len == 32) GAIB_FRD(8);
  else if (q.len == 64) GAIB_FRD(16);
  else GAIB_FRD(32);
#undef GAIB_FRD
  GAIB_LAUNCH_CHECK();
  return launch_alpha_grads<E, WIDE>(ctx, g->nv, q.len, q.heads, q.feat, ws.rs, ws.cs, ws.partial, q.alpha_lgrad, q.alpha_rgrad, q.ld);
}

// a public backward call: a.len / a.heads are the full row's
template <typename E>
int gat_backward_fused_seq(gaib_ctx* ctx, gaib_graph* g, GatBwd<E> a) {
  const char* who = a.who;
  const int len = a.len, heads = a.heads;
  constexpr bool fp32 = std::is_same<E, float>::value;
  GAIB_TRY(gat_check_call(who, ctx, g, len, heads, a.phase, a.drop, a.win));
  if (g->nv == 0) {
    if (a.rect) {  // a rank without rows: the decision of the ranks WITH rows (shape and option alone, see the forward); its zero
                   // alpha gradients are summed over the ranks afterwards
      if (!(gat_fused_shape(len, heads) && ctx->gat_fused_bwd != 0)) return gat_refuse(who, len, heads);
      if (a.phase == 0) return GAIB_OK;
    }
    return zero_alpha_grads(ctx, len, a.alpha_lgrad, a.alpha_rgrad);
  }
  GAIB_TRY(gat_check_ptrs(a));
  if (a.drop && g->nc != g->nv) return gat_refuse(who, len, heads);  // (no _rect form)
  GAIB_HIP(hipSetDevice(ctx->device));
  int w = len, rc = GAIB_OK;
  const int S = (a.rect || a.win || !a.row_stats) ? 1 : gat_wide_route(ctx, len, heads, &w);  // the row-statistics form only
  const int Hs = heads / S;
  const uintptr_t align_or = table_align(a.feat) | table_align(a.grad) | (uintptr_t)a.norm_scores | (uintptr_t)a.row_stats |
                             (uintptr_t)a.rec_tab | (uintptr_t)a.grad_out;
  if (!gat_fused_applies(ctx, g, w, Hs, ctx->gat_fused_bwd, align_or, &rc, a.rect)) return rc != GAIB_OK ? rc : gat_refuse(who, len, heads);
  // the reverse edge: p[rev e] where p is not formed again; under dropout its mask is the one of element rev(e) * heads + head
  if (a.drop || (!a.rect && !a.row_stats)) GAIB_TRY(gaib_graph_ensure_rev(ctx, g));
  GAIB_TRY(gaib_graph_ensure_chunks(ctx, g));
  a.strided = S >= 2 || a.win || (a.drop && !fp32);
  // the narrow undropped row-statistics calls: the packed-math sweep for heads of at most 16 lanes over a table below 4 GB (32-bit
  // byte offsets), else (fp32) the interleaved table; the other calls run the chunk kernel over the three separate tables
  const bool plain = S == 1 && !a.strided && !a.drop && !a.rect && a.row_stats;
  const int ldt = gat_packed_row<E>(len, heads), ldi = 2 * len + 4 * heads;
  const bool pk = plain && ctx->gat_bwd_pk == 1 && (len / 4) / heads <= 16 && (uint64_t)g->nv * (uint64_t)ldt * 4u < ((uint64_t)1 << 32);
  const bool inter = fp32 && plain && !pk && ctx->gat_interleave == 1;
  BwdWs ws;
  GAIB_TRY(gat_backward_ws(ctx, g, w, Hs, !a.rect, pk ? up4((size_t)g->nv * ldt) : inter ? up4((size_t)g->nv * ldi) : 0, &ws));
  ProfScope ps(ctx, "gat_bwd_fused", gat_prof_bytes_bwd(g, w, Hs, S), 8.0 * (double)g->ne * len);
  unsigned grid;
  int per_xcd;
  chunk_grid(ctx, g, !a.rect, &grid, &per_xcd);
  a.len = w, a.heads = Hs, a.ld = len, a.stats_ld = heads;
  a.unroll8 = !a.rect && ctx->gat_fused_unroll == 8;
  a.rec = a.rect ? reinterpret_cast<const f4*>(a.rec_tab) : ws.rec;
  a.rec_ld = a.rect ? heads : Hs;
  for (int s = 0; s < S; ++s) {
    GatBwd<E> q = a;
    DropWin dw = {};
    if (a.drop) dw = *a.drop, dw.mask_head0 += s * Hs, q.drop = &dw;
    q.feat += s * w, q.grad += s * w, q.alpha_l += s * w, q.alpha_r += s * w;
    q.grad_out += s * w, q.alpha_lgrad += s * w, q.alpha_rgrad += s * w;
    if (!a.rect) {
      q.fwd_out += s * w;
      if (q.row_stats) q.row_stats += 2 * s * Hs;
      GAIB_TRY(q.strided ? (gat_bwd_prologue<E, true>(ctx, g->nv, w, Hs, q.ld, q.stats_ld, q.grad, q.fwd_out, q.row_stats, ws.rowdot, ws.rec))
                         : (gat_bwd_prologue<E, false>(ctx, g->nv, w, Hs, q.ld, q.stats_ld, q.grad, q.fwd_out, q.row_stats, ws.rowdot, ws.rec)));
    }
    if (pk) GAIB_TRY(gat_bwd_sweep_packed(ctx, g, q, ws, grid, per_xcd));
    else if (!inter) GAIB_TRY(gat_bwd_sweep(ctx, g, q, ws, grid, per_xcd));
    else if constexpr (fp32) GAIB_TRY(gat_bwd_sweep_interleaved(ctx, g, q, ws, grid, per_xcd));
    if (q.phase == 0) return GAIB_OK;  // (_rect: the partials wait in the workspace for phase 1)
    GAIB_TRY(q.strided ? (gat_bwd_epilogue<E, true>(ctx, g, q, ws)) : (gat_bwd_epilogue<E, false>(ctx, g, q, ws)));
  }
  return GAIB_OK;
}

}  // namespace
