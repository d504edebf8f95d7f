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
// call would take one of them (short rows, a numbering with locality), the route function of spmm.hip refuses -- "the form this
// call would take has no packed gather" -- and the caller gathers dense.
// A 256-column table (gaib_pack_zs_wide: one 128-column image per K-slab) runs as the dense call's two K-slab launches, each of
// them the packed launch over its slab's image (E = zs_wide_t: the dense rows behind the image are 1024 B apart): one product,
// the 8-row strip or -- 256 outputs -- the 2-row strip, the second slab adding to y (launch_kslab_zs).
// No reference counterpart (the reference aggregates dense fp32 tables: include/gnn/graph_operations.h:8-178).
#include "spmm_kernels.h"

namespace {

// the launch of the form's kernel over E = zs_t / zs_wide_t, after launch_fused's own prologue
#define GAIB_ZS_LAUNCH(GM, STRIP, DUAL, YACC)                                                                              \
  do {                                                                                                                     \
    auto kern = spmm_gemm_kernel<2, WMODE, 16, GM, STRIP, DUAL, false, YACC, false, false, false, false, E>;               \
    GAIB_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));              \
    kern<<<dim3(fl.grid), FUSE_WAVES * 64, fl.lds, ctx->stream>>>(a, f);                                                   \
  } while (0)

// 128 columns in one launch: two products on the 2-row strip, or one on the 8-row strip (hot/cold where the form says so)
template <int WMODE>
int launch_fused_zs(gaib_ctx* ctx, const gaib_graph* g, const FuseForm& fm, SpmmArgs a, FuseArgs f, float* heavy_scratch) {
  typedef zs_t E;
  FusedLaunch fl;
  GAIB_TRY((fused_prologue<2, WMODE, false, E>(ctx, g, fm, a, f, heavy_scratch, &fl)));
  ProfScope ps(ctx, fl.key, fl.bytes, fl.flops, a.ncols);
  if (fm.dual) GAIB_ZS_LAUNCH(1, 2, true, false);
  else if (fm.hot_cold) {
    GAIB_ZS_LAUNCH(3, 8, false, false);
    ctx->spmm_hot_cold_launches++;
  } else GAIB_ZS_LAUNCH(1, 8, false, false);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// One K-slab of a 256-column aggregation over its slab image: one product on the form's strip, the later slab adding to y.
// a.in = the slab's image (a.ld = 96), a.in2 = the dense table at the slab's first column, a.ldo = 256; the heavy
// rows' aggregates go to heavy_scratch (= f.heavy_agg: hv + k0, row stride a.ldo) as in the dense slab launch.
template <int WMODE>
int launch_kslab_zs(gaib_ctx* ctx, const gaib_graph* g, const FuseForm& fm, SpmmArgs a, FuseArgs f, float* heavy_scratch) {
  typedef zs_wide_t E;
  FusedLaunch fl;
  GAIB_TRY((fused_prologue<2, WMODE, false, E>(ctx, g, fm, a, f, heavy_scratch, &fl)));
  ProfScope ps(ctx, fl.key, fl.bytes, fl.flops, a.ncols);
  if (fm.strip == 2) {
    if (fm.yacc) GAIB_ZS_LAUNCH(1, 2, false, true);
    else GAIB_ZS_LAUNCH(1, 2, false, false);
  } else {
    if (fm.yacc) GAIB_ZS_LAUNCH(1, 8, false, true);
    else GAIB_ZS_LAUNCH(1, 8, false, false);
  }
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}
#undef GAIB_ZS_LAUNCH

}  // namespace

int gaib_spmm_kslab_zs(gaib_ctx* ctx, const gaib_graph* g, const FuseForm& fm, const SpmmArgs& a, const FuseArgs& f, float* heavy_scratch, int wmode) {
  return wmode == 0 ? launch_kslab_zs<0>(ctx, g, fm, a, f, heavy_scratch) : launch_kslab_zs<1>(ctx, g, fm, a, f, heavy_scratch);
}

int gaib_spmm_fused_zs(gaib_ctx* ctx, const gaib_graph* g, const FuseForm& fm, const SpmmArgs& a, const FuseArgs& f, float* heavy_scratch, int wmode) {
  return wmode == 0 ? launch_fused_zs<0>(ctx, g, fm, a, f, heavy_scratch) : launch_fused_zs<1>(ctx, g, fm, a, f, heavy_scratch);
}
