// spmm_fp8.hip -- the row kernels of spmm_kernels.h (spmm_w64_kernel, spmm_heavy_kernel) instantiated for fp8 feature tables
// with per-row scales (E = fp8_t: OCP e4m3 "fn" bytes), whole graphs only:
//   out[i,:] (+)= sum_e (w_e * scale[col_e]) * f32(q[col_e,:])
// Only the gather and the weight a lane holds for its edge differ from the fp32 instantiations of spmm.hip: a quarter of the
// bytes per gathered row, held packed while in flight and widened exactly (v_cvt_pk_f32_fp8) where consumed; the power-of-two
// scale of the edge's column multiplied into the edge's weight next to the column id, once per edge.  The CSR order of a row's
// additions with separate multiply and add, the heavy threshold and its 16-wave LDS combine and every store are the fp32
// kernels' own, so out is bit-identical to gaib_spmm_ex on the widened table.  The entry point (gaib_spmm_fp8: checks, refusals,
// the ordered-chunk rule) stands in spmm.hip.
// No reference counterpart (the reference aggregates fp32 tables: src/gnn/gconv/gcn_aggregator.cpp:48-77).
// A translation unit of its own so that this set of instantiations compiles next to spmm.hip's.
#include "spmm_kernels.h"

namespace {

template <int WMODE>
int dispatch_fp8(gaib_ctx* ctx, const gaib_graph* g, const SpmmArgs& a0, int len) {
  // widest vector the row length, the row stride and the base pointers allow: VEC elements = VEC bytes per gather, 4 VEC bytes
  // per store (a lane never reaches past column len: the pad bytes behind it are not read).  A column's sum does not depend on
  // the lane width, so the choice is free: the narrowest lane that covers the row in one pass, as for bf16.
  const uintptr_t ai = (uintptr_t)a0.in, ao = (uintptr_t)a0.out;
  int vmax = 1;
  for (int v = 8; v > 1; v >>= 1)
    if (len % v == 0 && a0.ld % v == 0 && (ai & (uintptr_t)(v - 1)) == 0 && (ao & (uintptr_t)((v >= 4 ? 16 : 4 * v) - 1)) == 0) {
      vmax = v;
      break;
    }
  int vec = vmax;
  for (int v = 1; v < vmax; v <<= 1)
    if ((len + v - 1) / v <= 64) {
      vec = v;
      break;
    }
  // one launch covers up to 256 lanes of <= 2 elements, 128 of 4 or 64 of 8 (the accumulators are fp32: as for bf16); wider
  // rows in column slabs, each walking the edge list again
  const int slab = vec >= 4 ? 512 : 256 * vec;
  for (int c0 = 0; c0 < len; c0 += slab) {
    SpmmArgs a = a0;
    a.in = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(a0.in) + c0);
    a.out = a0.out + c0;
    if (a.in_bytes) a.in_bytes -= (uint32_t)c0;
    a.ncols = (len - c0 < slab) ? (len - c0) : slab;
    const int lanes = (a.ncols + vec - 1) / vec;
    const int ct = lanes <= 64 ? 1 : (lanes <= 128 ? 2 : 4);
    int rc;
    if (vec == 8) rc = launch_w64<8, 1, WMODE, fp8_t>(ctx, g, a);
    else if (vec == 4) rc = ct == 1 ? launch_w64<4, 1, WMODE, fp8_t>(ctx, g, a) : launch_w64<4, 2, WMODE, fp8_t>(ctx, g, a);
    else if (vec == 2) rc = ct == 1 ? launch_w64<2, 1, WMODE, fp8_t>(ctx, g, a)
                                    : (ct == 2 ? launch_w64<2, 2, WMODE, fp8_t>(ctx, g, a) : launch_w64<2, 4, WMODE, fp8_t>(ctx, g, a));
    else rc = ct == 1 ? launch_w64<1, 1, WMODE, fp8_t>(ctx, g, a)
                      : (ct == 2 ? launch_w64<1, 2, WMODE, fp8_t>(ctx, g, a) : launch_w64<1, 4, WMODE, fp8_t>(ctx, g, a));
    if (rc != GAIB_OK) return rc;
  }
  return GAIB_OK;
}

}  // namespace

int gaib_spmm_plain_fp8(gaib_ctx* ctx, const gaib_graph* g, const SpmmArgs& a, int wmode, int len) {
  switch (wmode) {
    case 0: return dispatch_fp8<0>(ctx, g, a, len);
    case 1: return dispatch_fp8<1>(ctx, g, a, len);
    case 2: return dispatch_fp8<2>(ctx, g, a, len);
    default:  // (defensive only: the fp8 entry points take no head count, so spmm_setup never hands them a multi-head mode)
      gaib_set_error("gaib_spmm_fp8: multi-head weights are not supported on fp8 tables");
      return GAIB_ERR_UNSUPPORTED;
  }
}
