// spmm_gemm_zs.hip -- the fused aggregation + dense product of spmm_kernels.h (spmm_gemm_kernel, spmm_heavy_kernel)
// instantiated for zero-suppressed feature tables (E = zs_t, spmm_core.h; packed by gaib_pack_zs), whole graphs only:
//   agg[i,:] = sum_e w_e * unpack(zs[col_e,:]) ;  y[i,:] = act(agg[i,:] . op(W) [+ rows2[i,:] . op(W2)])
// A relu-masked gradient is about half +0.0: packed, a row of 128 floats is three 128-B lines instead of four, and the
// aggregation's time follows the lines a gathered row touches.  Only the gather differs from the fp32 instantiations of spmm.hip:
// a row in flight is the two dwords a lane asked for, expanded with cross-lane permutes where it is consumed, four rows at a time (RowGather::zs_issue / zs_select);
// suppressed columns enter as +0.0, so every product w * x and every addition of the fp32 kernels is still made, in the same
// order: agg and y are bit-identical to gaib_spmm_gemm(2) on the dense table.
// Row forms only (8-row strip, or the 2-row strip with two products), per-row and per-edge weights, buffer addressing; the
// edge-stream forms, the XCD-affine tile supply, partitions and 64-bit addressing have no packed gather: where the dense
// call would take one of them (short rows, a numbering with locality), spmm_gemm_impl (spmm.hip) refuses and the caller gathers
// dense.
// A 256-column table (gaib_pack_zs_wide: one 128-column image per K-slab) runs as the dense call's two K-slab launches, each of
// them the packed launch over its slab's image (E = zs_wide_t: the dense rows behind the image are 1024 B apart): one product,
// the 8-row strip or -- 256 outputs -- the 2-row strip, the second slab adding to y (launch_kslab_zs).
// No reference counterpart (the reference aggregates dense fp32 tables: include/gnn/graph_operations.h:8-178).
#include "spmm_kernels.h"

namespace {

template <int WMODE>
int launch_fused_zs(gaib_ctx* ctx, const gaib_graph* g, SpmmArgs a, FuseArgs f, float* heavy_scratch) {
  constexpr int U = 16;
  constexpr int K = 128;
  const bool dual = f.wt2 != nullptr;
  // hot/cold gathers (option spmm_hot_cold; a.col_flagged set by spmm_gemm_impl): the one-product form and the heavy kernel next
  // to it; two products read the plain ids with the default policy
  const bool hot_cold = a.col_flagged && !dual;
  if (hot_cold) a.col = a.col_flagged;
  if (g->n_heavy > 0) {
    SpmmArgs h = a;
    h.row_list = g->heavy_rows;
    h.row_order = g->heavy_rows + g->n_heavy;
    h.out = heavy_scratch;
    h.compact = 1;
    h.relu = 0;
    h.accumulate = 0;
    const size_t lds = sizeof(float) * HEAVY_WAVES * K;
    // (bytes and flops are priced on the dense formula under the dense keys: a work rate in dense bytes)
    ProfScope ps(ctx, "spmm_heavy", gaib_alg_spmm_bytes((double)g->heavy_edges, (double)g->n_heavy, a.ncols, WMODE == 0 ? 0 : 4, 1),
                 2.0 * g->heavy_edges * a.ncols, a.ncols);
    if (hot_cold) spmm_heavy_kernel<2, 1, WMODE, U, 3, false, zs_t><<<dim3((unsigned)g->n_heavy), HEAVY_WAVES * 64, lds, ctx->stream>>>(h);
    else spmm_heavy_kernel<2, 1, WMODE, U, 1, false, zs_t><<<dim3((unsigned)g->n_heavy), HEAVY_WAVES * 64, lds, ctx->stream>>>(h);
    GAIB_LAUNCH_CHECK();
  }
  f.tile_xcd = 0;
  const int strip = dual ? 2 : 8;  // (checked by spmm_gemm_impl)
  const size_t lds = fuse_lds_bytes(K, f.n_out, dual, strip);
  const int64_t ntiles = cdiv64(a.n_rows, FUSE_ROWS);
  const int cus = ctx->spmm_fuse_cus > 0 ? ctx->spmm_fuse_cus : ctx->num_cus;
  const unsigned grid = (unsigned)std::min<int64_t>(cus, cdiv64(ntiles, FUSE_WAVES));
  GAIB_HIP(hipMemsetAsync(f.tile_counter, 0, 8 * sizeof(int), ctx->stream));
  const double e_l = (double)g->ne - (g->n_heavy > 0 ? (double)g->heavy_edges : 0.0), r_all = (double)a.n_rows;
  const double fused_bytes = gaib_alg_spmm_bytes(e_l, r_all, a.ncols, WMODE == 0 ? 0 : 4, (a.out ? 1 : 0) + (f.agg_in ? 1 : 0) + (dual ? 1 : 0)) +
                             r_all * 4.0 * f.n_out;
  const double fused_flops = 2.0 * e_l * a.ncols + 2.0 * r_all * a.ncols * f.n_out * (dual ? 2 : 1);
  ProfScope ps(ctx, "spmm_gemm_fused", fused_bytes, fused_flops, a.ncols);
  if (dual) {
    auto kern = spmm_gemm_kernel<2, WMODE, U, 1, 2, true, false, false, false, false, false, false, zs_t>;
    GAIB_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    kern<<<dim3(grid), FUSE_WAVES * 64, lds, ctx->stream>>>(a, f);
  } else if (hot_cold) {
    auto kern = spmm_gemm_kernel<2, WMODE, U, 3, 8, false, false, false, false, false, false, false, zs_t>;
    GAIB_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    kern<<<dim3(grid), FUSE_WAVES * 64, lds, ctx->stream>>>(a, f);
    ctx->spmm_hot_cold_launches++;
  } else {
    auto kern = spmm_gemm_kernel<2, WMODE, U, 1, 8, false, false, false, false, false, false, false, zs_t>;
    GAIB_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    kern<<<dim3(grid), FUSE_WAVES * 64, lds, ctx->stream>>>(a, f);
  }
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// One K-slab of a 256-column aggregation over its slab image: launch_fused's y_accum / strip choices (spmm_kernels.h) with the
// packed gather.  a.in = the slab's image (a.ld = 96), a.in2 = the dense table at the slab's first column, a.ldo = 256; the heavy
// rows' aggregates go to heavy_scratch (= f.heavy_agg: hv + k0, row stride a.ldo) as in the dense slab launch.
template <int WMODE>
int launch_kslab_zs(gaib_ctx* ctx, const gaib_graph* g, SpmmArgs a, FuseArgs f, float* heavy_scratch) {
  constexpr int U = 16;
  constexpr int K = 128;
  if (g->n_heavy > 0) {
    SpmmArgs h = a;
    h.row_list = g->heavy_rows;
    h.row_order = g->heavy_rows + g->n_heavy;
    h.out = heavy_scratch;
    h.compact = 1;
    h.relu = 0;
    h.accumulate = 0;
    const size_t lds = sizeof(float) * HEAVY_WAVES * K;
    ProfScope ps(ctx, "spmm_heavy", gaib_alg_spmm_bytes((double)g->heavy_edges, (double)g->n_heavy, a.ncols, WMODE == 0 ? 0 : 4, 1),
                 2.0 * g->heavy_edges * a.ncols, a.ncols);
    spmm_heavy_kernel<2, 1, WMODE, U, 1, false, zs_wide_t><<<dim3((unsigned)g->n_heavy), HEAVY_WAVES * 64, lds, ctx->stream>>>(h);
    GAIB_LAUNCH_CHECK();
  }
  f.tile_xcd = 0;
  const int strip = fuse_strip_rows(K, f.n_out, false);  // 8 or 2 (checked by spmm_gemm_impl)
  const size_t lds = fuse_lds_bytes(K, f.n_out, false, strip);
  const int64_t ntiles = cdiv64(a.n_rows, FUSE_ROWS);
  const int cus = ctx->spmm_fuse_cus > 0 ? ctx->spmm_fuse_cus : ctx->num_cus;
  const unsigned grid = (unsigned)std::min<int64_t>(cus, cdiv64(ntiles, FUSE_WAVES));
  GAIB_HIP(hipMemsetAsync(f.tile_counter, 0, 8 * sizeof(int), ctx->stream));
  const double e_l = (double)g->ne - (g->n_heavy > 0 ? (double)g->heavy_edges : 0.0), r_all = (double)a.n_rows;
  const double fused_bytes = gaib_alg_spmm_bytes(e_l, r_all, a.ncols, WMODE == 0 ? 0 : 4, (a.out ? 1 : 0) + (f.agg_in ? 1 : 0)) +
                             r_all * 4.0 * f.n_out * (f.y_accum ? 2 : 1);
  const double fused_flops = 2.0 * e_l * a.ncols + 2.0 * r_all * a.ncols * f.n_out;
  ProfScope ps(ctx, "spmm_gemm_fused", fused_bytes, fused_flops, a.ncols);
#define GAIB_KSLAB_ZS(STRIP, YACC)                                                                                         \
  do {                                                                                                                     \
    auto kern = spmm_gemm_kernel<2, WMODE, U, 1, STRIP, false, false, YACC, false, false, false, false, zs_wide_t>;        \
    GAIB_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));              \
    kern<<<dim3(grid), FUSE_WAVES * 64, lds, ctx->stream>>>(a, f);                                                         \
  } while (0)
  if (strip == 2) {
    if (f.y_accum) GAIB_KSLAB_ZS(2, true);
    else GAIB_KSLAB_ZS(2, false);
  } else {
    if (f.y_accum) GAIB_KSLAB_ZS(8, true);
    else GAIB_KSLAB_ZS(8, false);
  }
#undef GAIB_KSLAB_ZS
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

}  // namespace

int gaib_spmm_kslab_zs(gaib_ctx* ctx, const gaib_graph* g, const void* spmm_args, const void* fuse_args, float* heavy_scratch,
                       int wmode) {
  const SpmmArgs& a = *static_cast<const SpmmArgs*>(spmm_args);
  const FuseArgs& f = *static_cast<const FuseArgs*>(fuse_args);
  return wmode == 0 ? launch_kslab_zs<0>(ctx, g, a, f, heavy_scratch) : launch_kslab_zs<1>(ctx, g, a, f, heavy_scratch);
}

int gaib_spmm_fused_zs(gaib_ctx* ctx, const gaib_graph* g, const void* spmm_args, const void* fuse_args, float* heavy_scratch,
                       int wmode) {
  const SpmmArgs& a = *static_cast<const SpmmArgs*>(spmm_args);
  const FuseArgs& f = *static_cast<const FuseArgs*>(fuse_args);
  return wmode == 0 ? launch_fused_zs<0>(ctx, g, a, f, heavy_scratch) : launch_fused_zs<1>(ctx, g, a, f, heavy_scratch);
}
