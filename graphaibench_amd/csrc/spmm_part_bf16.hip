// spmm_part_bf16.hip -- the row-class kernels of spmm_part.hip (PART = true: row map on out / agg / rows2 / y, column ids >=
// n_first index a second table) instantiated for bf16 feature tables (E = uint16_t: raw bf16 bits in BOTH tables):
//   out[map[i],:] (+)= sum_e w_e * widen(col_e < n_first ? in[col_e,:] : in2[col_e - n_first,:])
// Only the gather differs from the fp32 class kernels: half the bytes per gathered row against whichever of the two buffer
// descriptors the (wave-uniform) column id selects -- or the 64-bit path --, held as the packed words it arrived in and widened
// exactly (bits << 16) where it is consumed.  Weights, the CSR order of a row's additions with separate multiply and add, the heavy
// threshold and its 16-wave LDS combine, the GAIB_ACCUMULATE continuation, op(W) in LDS, the MFMA loop and every store are the
// fp32 kernels' own, and the route is chosen on the fp32 sizes (gemm_route, spmm.hip): results are bit-identical to
// gaib_spmm_ex / gaib_spmm_2t / gaib_spmm_gemm_2t on the tables widened to fp32.
// No reference counterpart (the reference has no multi-GPU GNN and aggregates fp32 tables:
// src/gnn/gconv/gcn_aggregator.cpp:48-77; the partition structure is src/partitioner/graph_partition.cc:70-80,128-178).
// A translation unit of its own so that this set of instantiations compiles beside spmm.hip, spmm_part.hip and spmm_gemm_bf16.hip.
#include "spmm_kernels.h"

namespace {

typedef uint16_t bf16_t;

template <int VEC, int CT, int WMODE>
int part_w64_bf16(gaib_ctx* ctx, const gaib_graph* g, const SpmmArgs& a) {
  constexpr int U = (VEC * CT >= 8) ? 4 : (VEC * CT >= 4 ? 8 : 16);  // as launch_w64
  const bool buf = a.in_bytes != 0 && ctx->spmm_addr_mode != 2 && (!a.in2 || a.in2_bytes != 0);
  return buf ? launch_w64_u<VEC, CT, WMODE, U, 1, true, bf16_t>(ctx, g, a) : launch_w64_u<VEC, CT, WMODE, U, 0, true, bf16_t>(ctx, g, a);
}

// lane vector by width, the rule of dispatch_bf16 (spmm.hip): one row per wave, the narrowest vector that covers the row in one
// pass -- VEC elements are 2 VEC bytes per gather and 4 VEC bytes per store.  A row's sum does not depend on the choice.
template <int WMODE>
int part_vec_bf16(gaib_ctx* ctx, const gaib_graph* g, const SpmmArgs& a0, int len) {
  const uintptr_t ai = (uintptr_t)a0.in | (uintptr_t)a0.in2, ao = (uintptr_t)a0.out;
  int vmax = 1;
  for (int v = 8; v > 1; v >>= 1)
    if (len % v == 0 && (ai & (2 * v - 1)) == 0 && (ao & ((v >= 4 ? 16 : 4 * v) - 1)) == 0) {
      vmax = v;
      break;
    }
  int vec = vmax;
  for (int v = 1; v < vmax; v <<= 1)
    if ((len + v - 1) / v <= 64) {
      vec = v;
      break;
    }
  // one launch covers up to 256 lanes of <= 2 elements, 128 of 4 or 64 of 8; wider rows in column slabs
  const int slab = vec >= 4 ? 512 : 256 * vec;
  for (int c0 = 0; c0 < len; c0 += slab) {
    SpmmArgs a = a0;
    a.in = reinterpret_cast<const float*>(reinterpret_cast<const bf16_t*>(a0.in) + c0);
    if (a0.in2) a.in2 = reinterpret_cast<const float*>(reinterpret_cast<const bf16_t*>(a0.in2) + c0);
    a.out = a0.out + c0;
    a.ncols = (len - c0 < slab) ? (len - c0) : slab;
    if (a.in_bytes) a.in_bytes -= (uint32_t)(2 * c0);
    if (a.in2_bytes) a.in2_bytes -= (uint32_t)(2 * c0);
    const int lanes = (a.ncols + vec - 1) / vec;
    const int ct = lanes <= 64 ? 1 : (lanes <= 128 ? 2 : 4);
    int rc;
    if (vec == 8) rc = part_w64_bf16<8, 1, WMODE>(ctx, g, a);
    else if (vec == 4) rc = ct == 1 ? part_w64_bf16<4, 1, WMODE>(ctx, g, a) : part_w64_bf16<4, 2, WMODE>(ctx, g, a);
    else if (vec == 2) rc = ct == 1 ? part_w64_bf16<2, 1, WMODE>(ctx, g, a)
                                    : (ct == 2 ? part_w64_bf16<2, 2, WMODE>(ctx, g, a) : part_w64_bf16<2, 4, WMODE>(ctx, g, a));
    else rc = ct == 1 ? part_w64_bf16<1, 1, WMODE>(ctx, g, a)
                      : (ct == 2 ? part_w64_bf16<1, 2, WMODE>(ctx, g, a) : part_w64_bf16<1, 4, WMODE>(ctx, g, a));
    if (rc != GAIB_OK) return rc;
  }
  return GAIB_OK;
}

}  // namespace

int gaib_spmm_part_plain_bf16(gaib_ctx* ctx, const gaib_graph* g, const SpmmArgs& a, int wmode, int len) {
  return wmode == 0 ? part_vec_bf16<0>(ctx, g, a, len) : part_vec_bf16<1>(ctx, g, a, len);
}

// row forms with 8- and 2-row strips, two products, the edge stream in batches and as a software pipeline; gathers in flight as
// in the whole-graph bf16 kernels (launch_fused).  No XCD-affine variants, as for every PART instantiation.
int gaib_spmm_part_fused_bf16(gaib_ctx* ctx, const gaib_graph* g, const FuseForm& fm, const SpmmArgs& a, const FuseArgs& f, float* heavy_scratch, int wmode) {
  if (fm.vec == 1)
    return wmode == 0 ? launch_fused<1, 0, true, bf16_t>(ctx, g, fm, a, f, heavy_scratch)
                      : launch_fused<1, 1, true, bf16_t>(ctx, g, fm, a, f, heavy_scratch);
  return wmode == 0 ? launch_fused<2, 0, true, bf16_t>(ctx, g, fm, a, f, heavy_scratch)
                    : launch_fused<2, 1, true, bf16_t>(ctx, g, fm, a, f, heavy_scratch);
}
