// spmm_gemm_fp8.hip -- the fused aggregation + dense product of spmm_kernels.h (spmm_gemm_kernel, spmm_heavy_kernel)
// instantiated for fp8 feature tables with per-row scales (E = fp8_t: OCP e4m3 "fn" bytes), whole graphs only:
//   agg[i,:] = sum_e (w_e * scale[col_e]) * f32(q[col_e,:]) ;  y[i,:] = act(agg[i,:] . op(W) [+ rows2[i,:] . op(W2)])
// Only the gather and the weight a lane holds for its edge differ from the fp32 instantiations of spmm.hip (see spmm_fp8.hip);
// partial sums, op(W) in LDS, the MFMA loop and every store are the fp32 kernels' own, so agg and y are bit-identical to
// gaib_spmm_gemm on the widened table.  The route (fused, two K-slabs, fused + accumulating GEMM, two kernels) is chosen by the
// route function of spmm.hip (gemm_route) on what the fp32 call would see; the form has the global tile counter and no hot/cold
// gather, as for bf16.
// No reference counterpart (the reference aggregates and multiplies fp32 tables in separate passes:
// src/gnn/gconv/gcn_aggregator.cpp:48-77, include/gnn/graph_operations.h:8-178).
// A translation unit of its own so that this set of instantiations compiles next to spmm.hip's.
#include "spmm_kernels.h"

int gaib_spmm_fused_fp8(gaib_ctx* ctx, const gaib_graph* g, const FuseForm& fm, const SpmmArgs& a, const FuseArgs& f, float* heavy_scratch, int wmode) {
  if (fm.vec == 1)
    return wmode == 0 ? launch_fused<1, 0, false, fp8_t>(ctx, g, fm, a, f, heavy_scratch)
                      : launch_fused<1, 1, false, fp8_t>(ctx, g, fm, a, f, heavy_scratch);
  return wmode == 0 ? launch_fused<2, 0, false, fp8_t>(ctx, g, fm, a, f, heavy_scratch)
                    : launch_fused<2, 1, false, fp8_t>(ctx, g, fm, a, f, heavy_scratch);
}
