// spmm_core.h -- device code shared by the aggregation kernels (spmm.hip, spmm_part.hip, spmm_part_bf16.hip, spmm_gemm_bf16.hip, spmm_fp8.hip,
// spmm_gemm_fp8.hip):
// launch arguments, the feature-row gather and the per-wave edge loop.
#pragma once
#include <type_traits>
#include "common.h"

// (outside the unnamed namespace: the launchers declared in spmm_kernels.h pass it by reference between translation units)
struct SpmmArgs {
  const int64_t* rowptr;
  const uint32_t* col;
  const float* rw;      // per-row weight    (WMODE 0)
  const float* ew;      // per-edge weight   (WMODE 1, 2)
  const uint32_t* rev;  // reverse edge ids  (WMODE 2: w = ew[rev[e]])
  const float* in;
  float* out;
  int64_t ld;   // row stride of the gathered table `in` (floats)
  int64_t ldo;  // row stride of out, of the partial sums continued in accumulate mode and of the fused path's row operands
  int ncols;   // columns handled by this launch (<= 64*VEC*CT), starting at in/out
  int n_rows;
  int heavy_thr;
  const uint32_t* row_list;  // heavy kernel only: row ids (ascending) ...
  const uint32_t* row_order; // ... and the slot each workgroup takes (longest rows first)
  int nblocks;               // light kernels: logical number of row blocks
  int per_xcd;               // ceil(nblocks/8) when swizzled, 0 otherwise
  int xcd_chunk;             // > 0: an XCD takes chunks of this many consecutive row blocks in round robin over the XCDs
                             // (0: one contiguous range of row blocks per XCD)
  uint32_t in_bytes;         // BUF kernels: size of the feature table (< 4 GB)
  const uint32_t* col_flagged;  // GM 3: column ids with the top bit set on cold columns
  int accumulate;            // out += instead of out = (second half of a split aggregation)
  int relu;                  // clamp at 0 on store (activation fused)
  int heads;                 // WMODE 3/4: edge weights are [ne][heads]; head of a column = col / dh
  int dh;
  int compact;               // heavy kernel: row k of row_list is written to out row k (fused path's scratch)
  int col0;                  // WMODE 3/4: column of the whole row at which in / out start (a column slab of dispatch_vec; else 0)
                             // (in what was padding ahead of row_map: no other field moves, the struct keeps its size)
  // PART kernels (row classes of a vertex-range partition, spmm_part.hip) -- ignored by the others:
  const uint32_t* row_map;   // row r of the graph is row row_map[r] of out / the continued partial sums / rows2 / y (NULL: r itself)
  const float* in2;          // column ids >= n_first index this second table (row id - n_first): the halo table behind the
  uint32_t n_first;          //   rank's own rows.  in2 == NULL: one table, n_first = 0xffffffff
  uint32_t in2_bytes;        // BUF kernels: size of the second table (< 4 GB; of its bf16 bits when the tables are bf16)
  // fp8 tables (E = fp8_t; never PART): in2 points at the table's row scales, float[nc] (see fp8_scales)
};

namespace {

// the row of the caller's matrices that row r of the graph stands for
template <bool PART>
__device__ __forceinline__ int64_t out_row(const SpmmArgs& a, int64_t r) {
  if constexpr (PART) return a.row_map ? (int64_t)a.row_map[r] : r;
  else return r;
}

template <int VEC> struct VecT;
template <> struct VecT<1> { typedef float type; };
template <> struct VecT<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct VecT<4> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct VecT<8> { typedef float type __attribute__((ext_vector_type(8))); };  // (bf16 tables: one 16-B gather)

template <int VEC>
__device__ __forceinline__ typename VecT<VEC>::type vzero() {
  typename VecT<VEC>::type z;
  if constexpr (VEC == 1) z = 0.f;
  else
    for (int i = 0; i < VEC; ++i) z[i] = 0.f;
  return z;
}
template <int VEC>
__device__ __forceinline__ typename VecT<VEC>::type vrelu(typename VecT<VEC>::type v) {
  if constexpr (VEC == 1) return v > 0.f ? v : 0.f;
  else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = v[i] > 0.f ? v[i] : 0.f;
    return v;
  }
}
template <int VEC>
__device__ __forceinline__ void vacc(typename VecT<VEC>::type& acc, float w,
                                     const typename VecT<VEC>::type& x) {
  // separate multiply and add: the reference does scale() then vadd_cpu()
  // (math_functions.cpp:336-356, 266-283); this file is built with -ffp-contract=off.
  if constexpr (VEC == 1) {
    float t = w * x;
    acc = acc + t;
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      float t = w * x[i];
      acc[i] = acc[i] + t;
    }
  }
}

// blockIdx -> row block.  Workgroups are dealt to the 8 XCDs round robin (XCD = blockIdx & 7), each XCD has its own L2.
//   per_xcd > 0, xcd_chunk == 0: XCD x owns the contiguous range [x * per_xcd, (x + 1) * per_xcd) of row blocks --
//     consecutive row blocks share an L2, but a graph whose long rows sit together (a degree-sorted numbering) loads
//     one XCD with most of the edges (scripts/locality_study.py --order degree: 2.5x slower);
//   xcd_chunk = C: XCD x takes the chunks x, x + 8, x + 16, ... of C consecutive row blocks -- still C consecutive
//     row blocks per L2 at a time, and the edges spread over the XCDs at C-block granularity.
__device__ __forceinline__ int logical_block(const SpmmArgs& a) {
  int b = blockIdx.x;
  if (a.per_xcd > 0) {
    const int x = b & 7, k = b >> 3;
    if (a.xcd_chunk > 0) b = ((k / a.xcd_chunk) * 8 + x) * a.xcd_chunk + (k % a.xcd_chunk);
    else b = x * a.per_xcd + k;
  }
  return b;
}

// WMODE: 0 per-row weight | 1 per-edge | 2 per-edge through the reverse permutation |
//        3 per-(edge, head) | 4 per-(edge, head) through the reverse permutation
template <int WMODE>
__device__ __forceinline__ float load_edge_w(const SpmmArgs& a, int64_t e, int head = 0) {
  if constexpr (WMODE == 1) return a.ew[e];
  else if constexpr (WMODE == 2) return a.ew[a.rev[e]];
  else if constexpr (WMODE == 3) return a.ew[e * a.heads + head];
  else if constexpr (WMODE == 4) return a.ew[(int64_t)a.rev[e] * a.heads + head];
  else return 0.f;
}

typedef unsigned u2_t __attribute__((ext_vector_type(2)));
typedef unsigned u4_t __attribute__((ext_vector_type(4)));

// bf16 tables (E = uint16_t: raw bf16 bits): VEC elements arrive in VEC / 2 dwords and are widened exactly (bits << 16);
// everything after the gather -- weights, sums, order, the fp32 output -- is the fp32 kernels' own.
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
template <int VEC> struct Bf16Raw;  // the packed words of VEC bf16 elements
template <> struct Bf16Raw<1> { typedef unsigned short type; };
template <> struct Bf16Raw<2> { typedef unsigned type; };
template <> struct Bf16Raw<4> { typedef u2_t type; };
template <> struct Bf16Raw<8> { typedef u4_t type; };
template <int VEC>
__device__ __forceinline__ typename VecT<VEC>::type widen_bf16(typename Bf16Raw<VEC>::type r) {
  typename VecT<VEC>::type v;
  if constexpr (VEC == 1) v = __uint_as_float((unsigned)r << 16);
  else if constexpr (VEC == 2) {
    v[0] = bf16_lo(r);
    v[1] = bf16_hi(r);
  } else {
#pragma unroll
    for (int i = 0; i < VEC / 2; ++i) {
      v[2 * i] = bf16_lo(r[i]);
      v[2 * i + 1] = bf16_hi(r[i]);
    }
  }
  return v;
}
// fp8 tables (E = fp8_t: OCP e4m3 "fn" bytes): VEC elements arrive in VEC bytes and are widened exactly by
// v_cvt_pk_f32_fp8 / v_cvt_f32_fp8.  A row r of the table stands for f32(q[r][:]) * scale[r] with scale[r] a power of two: the
// scale never touches the VEC x CT gathered elements -- it is folded into the edge's weight, w_e * scale[col_e] (an exact
// product while it stays a normal number, and one that commutes with the rounding of w * x), fetched per lane next to the
// column id and weight of a 64-edge chunk and consumed through the same readlane.  Everything after the gather is the fp32
// kernels' own, as for bf16.
struct fp8_t { uint8_t bits; };
template <int VEC> struct Fp8Raw;  // the packed bytes of VEC fp8 elements
template <> struct Fp8Raw<1> { typedef unsigned char type; };
template <> struct Fp8Raw<2> { typedef unsigned short type; };
template <> struct Fp8Raw<4> { typedef unsigned type; };
template <> struct Fp8Raw<8> { typedef u2_t type; };
template <int VEC>
__device__ __forceinline__ typename VecT<VEC>::type widen_fp8(typename Fp8Raw<VEC>::type r) {
  typename VecT<VEC>::type v;
  if constexpr (VEC == 1) v = __builtin_amdgcn_cvt_f32_fp8((int)(unsigned)r, 0);
  else if constexpr (VEC == 2) v = __builtin_amdgcn_cvt_pk_f32_fp8((int)(unsigned)r, false);
  else {
#pragma unroll
    for (int i = 0; i < VEC / 4; ++i) {
      unsigned w;
      if constexpr (VEC == 4) w = r;
      else w = r[i];
      const typename VecT<2>::type lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
      v[4 * i] = lo[0];
      v[4 * i + 1] = lo[1];
      v[4 * i + 2] = hi[0];
      v[4 * i + 3] = hi[1];
    }
  }
  return v;
}
// the row scales of an fp8 table (SpmmArgs::in2) and the weight lane l of a 64-edge chunk holds for its edge: w_e * scale[col_e]
// (WMODE 0 at a fixed row: roww * scale[col_e]).  c is the lane's column id as loaded -- under gather mode 3 its top bit is the
// hot/cold flag and is masked before it indexes the scales.
__device__ __forceinline__ const float* fp8_scales(const SpmmArgs& a) { return a.in2; }
template <int GM>
__device__ __forceinline__ float fp8_fold_scale(const SpmmArgs& a, uint32_t c, float w) {
  return w * fp8_scales(a)[GM == 3 ? (c & 0x7fffffffu) : c];
}
// the weight of edge idx of a 64-edge chunk in the edge-stream forms, where the row (and its weight roww) changes along the
// stream: an fp8 table's lanes hold w_e * scale[col_e], under WMODE 0 the scale alone -- roww * scale[col_e], one exact product
// per edge, never one per gathered element
template <int WMODE, bool F8>
__device__ __forceinline__ float stream_w(float roww, float w, int idx) {
  if constexpr (F8 && WMODE == 0) return roww * readlane_f(w, idx);
  else return (WMODE == 0) ? roww : readlane_f(w, idx);
}
// VEC elements of type E at p (global address) as VEC floats
template <int VEC, typename E>
__device__ __forceinline__ typename VecT<VEC>::type load_elems(const char* p) {
  if constexpr (sizeof(E) == 4) return *reinterpret_cast<const typename VecT<VEC>::type*>(p);
  else if constexpr (sizeof(E) == 1) return widen_fp8<VEC>(*reinterpret_cast<const typename Fp8Raw<VEC>::type*>(p));
  else return widen_bf16<VEC>(*reinterpret_cast<const typename Bf16Raw<VEC>::type*>(p));
}

// Zero-suppressed tables (E = zs_t; gaib_pack_zs, elementwise.hip): a row of 128 floats is 384 B on a 128-B boundary --
//   dwords 0-1  M0: bit l set when column 2l holds anything but bit pattern 0        dwords 2-3  M1: the same for column 2l + 1
//   dword 4 + 2k  the k-th kept value of the even columns (M0, in lane order)        dword 5 + 2k  the k-th of the odd columns (M1)
// i.e. the 8-B load of lane 2 + k holds the k-th value of either half, which is what lets the gather find a lane's two values
// with ONE cross-lane read each and no choice between a lane's two dwords (see zs_issue).  Either half holds up to GAIB_ZS_CAP
// values; a row with more in one half keeps only its masks there and is read from the dense table.  Unpacking reproduces every bit.
struct zs_t { uint32_t bits; };
constexpr int GAIB_ZS_ROW_BYTES = 384;
constexpr int GAIB_ZS_CAP = 46;
// E = zs_wide_t: one 128-column slab of a 256-column table (gaib_pack_zs_wide: one image per slab, each in the format above).  The
// packed gather is zs_t's; only the dense table behind it differs: its rows are 1024 B apart, and a.in2 points at the slab's first
// column, so an over-capacity half row is read at col * 1024 + the lane's offset.
struct zs_wide_t { uint32_t bits; };
template <typename E> struct ZsTraits { static constexpr bool zs = false; static constexpr uint32_t dense_row_bytes = 0u; };
template <> struct ZsTraits<zs_t> { static constexpr bool zs = true; static constexpr uint32_t dense_row_bytes = 512u; };
template <> struct ZsTraits<zs_wide_t> { static constexpr bool zs = true; static constexpr uint32_t dense_row_bytes = 1024u; };

// One feature-row gather.  BUF: `buffer_load_dwordxN v, voff, s[rsrc], soff offen` -- the row
// base (col * row bytes) is a 32-bit SGPR offset against one descriptor for the whole table,
// so a gather in flight costs only its VEC destination VGPRs (no 64-bit VGPR address pair).
// Needs the table to be < 4 GB; larger tables use 64-bit global_load addresses.
// GM (gather mode): 0 = 64-bit global_load; 1 = buffer_load, default cache policy; 2 = buffer_load nt
// (streaming) for every gather; 3 = buffer_load, nt only for COLD columns (top bit of the column id
// set by gaib_graph_ensure_hot_flags), so the hot rows keep their place in the caches -- the 4 MB L2 for the unfused kernels'
// 3 MB hot set (spmm_gather_mode 3), the Infinity Cache for the fused, heavy and packed launches' (spmm_hot_cold).  Every user of
// a column id of such a kernel masks the bit first; on a zero-suppressed table the bit chooses the policy of the packed
// three-line load and of an over-capacity row's dense load alike.
// PART: two tables -- column ids below n_first index `in`, the others `in2` (a rank's own rows and its halo table, which
// live in different allocations); the choice is a scalar select on the (wave-uniform) column id.  Both tables hold the same
// element type: fp32, or bf16 (spmm_part_bf16.hip) -- ldb, the n_first bias of inb2 and both descriptors then count bf16 bytes.
// E: element type of the table -- float, or uint16_t for a bf16 table (a.in then points at bf16 bits, a.ld counts
// elements, a.in_bytes is the bf16 size; voff is a byte offset into such a row); or zs_t for a zero-suppressed table (a.in
// then points at the packed rows, a.ld = 96, a.in_bytes is the packed size, and a.in2 / a.in2_bytes name the dense table the
// packed one was made from; voff is the lane's byte offset into the DENSE row, 8 * lane); or zs_wide_t for one slab of a wide
// zero-suppressed table (the same, with dense rows 1024 B apart).
template <int VEC, int GM, bool PART = false, typename E = float>
struct RowGather {
  static constexpr bool BUF = GM != 0;
  static constexpr bool ZS = ZsTraits<E>::zs;
  static_assert(!PART || !ZS, "two-table gathers: fp32 or bf16 tables");
  static_assert(!ZS || (VEC == 2 && (GM == 1 || GM == 3)), "zero-suppressed tables: 8-byte lanes (128 columns), buffer addressing");
  __amdgpu_buffer_rsrc_t rsrc, rsrc2;
  const char *inb, *inb2;  // inb2 is biased by -n_first rows: row base = inb2 + col * ldb
  int64_t ldb;
  uint32_t n_first;
  __device__ __forceinline__ RowGather(const SpmmArgs& a) {
    inb = reinterpret_cast<const char*>(a.in);
    ldb = a.ld * (int64_t)sizeof(E);
    if constexpr (BUF) rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, (int)a.in_bytes, 0x00020000);
    if constexpr (PART) {
      n_first = a.in2 ? a.n_first : 0xffffffffu;
      inb2 = reinterpret_cast<const char*>(a.in2) - (int64_t)a.n_first * ldb;
      if constexpr (BUF) rsrc2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.in2, 0, (int)a.in2_bytes, 0x00020000);
    }
    if constexpr (ZS) rsrc2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.in2, 0, (int)a.in2_bytes, 0x00020000);  // the dense table
  }
  // What a gather leaves in registers until it is consumed: the fp32 vector itself, or the packed words of VEC bf16 elements
  // (half the registers).  load_raw() requests, widen() -- exact, bits << 16 -- belongs at the point of use: widened at the load,
  // the shifts sit between the loads of a batch and every gather in flight holds fp32-sized registers.
  // A zero-suppressed gather is held as the two dwords the lane asked for (lanes 0 .. 47 cover the 384-B row).
  // An fp8 gather is held as the VEC bytes it arrived in (a quarter of the registers) and widened by v_cvt_pk_f32_fp8 at the same point.
  static constexpr bool F8 = sizeof(E) == 1;
  static_assert(!PART || !F8, "two-table gathers: fp32 or bf16 tables");
  typedef typename std::conditional<F8, typename Fp8Raw<VEC>::type, typename VecT<VEC>::type>::type wide_raw_t;
  typedef typename std::conditional<ZS, u2_t, typename std::conditional<sizeof(E) == 2, typename Bf16Raw<VEC>::type,
                                                                           wide_raw_t>::type>::type raw_t;
  static __device__ __forceinline__ typename VecT<VEC>::type widen(const raw_t& r) {
    static_assert(!ZS, "zero-suppressed tables are expanded by zs_issue / zs_select");
    if constexpr (sizeof(E) == 2) return widen_bf16<VEC>(r);
    else if constexpr (F8) return widen_fp8<VEC>(r);
    else return r;
  }
  // Expansion of a zero-suppressed row where it is consumed.  Control flow is wave-uniform here and every lane is live: the masks
  // come from lanes 0 and 1; a lane's even column is component 0 of lane 2 + (set bits of M0 below the lane), its odd column
  // component 1 of lane 2 + (set bits of M1 below the lane) -- one ds_bpermute each (no LDS is allocated); suppressed columns are
  // +0.0 by a select with the mask itself as its lane mask.  Per row: 4 readlane, 4 mbcnt, 2 shifts, 2 selects next to the dense
  // loop's 2 multiplies and 2 adds.  A row with more than GAIB_ZS_CAP values in a half holds only its masks: it is read from the
  // dense table, 512 B per row, and waited for.
  // The expansion runs in two phases, for a GROUP of rows (wave_accumulate): the cross-lane reads of every row of the group are
  // issued back to back and travel together, instead of one round trip after the other with a branch in between.
  // zs_issue: masks to SGPRs, ranks, and the two permutes (p holds garbage above the masks' set bits and on an over-capacity
  // row).  The capacity test stays on the scalar unit: a popcount is at most 64, so bit 6 of popcount + (63 - GAIB_ZS_CAP) says
  // "more than GAIB_ZS_CAP"; the group ORs these sums and branches once (zs_over).
  typedef unsigned long long zs_mask_t;
  static __device__ __forceinline__ uint32_t zs_over_bits(zs_mask_t m0, zs_mask_t m1) {
    return ((uint32_t)__builtin_popcountll(m0) + (uint32_t)(63 - GAIB_ZS_CAP)) | ((uint32_t)__builtin_popcountll(m1) + (uint32_t)(63 - GAIB_ZS_CAP));
  }
  static __device__ __forceinline__ bool zs_over(uint32_t over) { return (over & 64u) != 0; }
  static __device__ __forceinline__ void zs_issue(const raw_t& r, raw_t& p, zs_mask_t& m0, zs_mask_t& m1, uint32_t& over) {
    m0 = ((zs_mask_t)(uint32_t)__builtin_amdgcn_readlane((int)r[1], 0) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)r[0], 0);
    m1 = ((zs_mask_t)(uint32_t)__builtin_amdgcn_readlane((int)r[1], 1) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)r[0], 1);
    over |= zs_over_bits(m0, m1);
    const uint32_t l0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 2u));
    const uint32_t l1 = __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 2u));
    p[0] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(l0 << 2), (int)r[0]);
    p[1] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(l1 << 2), (int)r[1]);
  }
  // zs_fix: the rare path, entered for a whole group when any of its rows is over capacity.  Such a row is read from the dense
  // table, 512 B (of a row ZsTraits<E>::dense_row_bytes long), and waited for; the others are selected as on the fast path.  It returns the row rather than repairing
  // registers and masks for a select shared with the fast path: values that join after the branch cost the FAST path a copy
  // of every register and mask of the group, and a wait for the dense load left to the join would drain the gathers in flight.
  __device__ __forceinline__ typename VecT<VEC>::type zs_fix(const raw_t& p, zs_mask_t m0, zs_mask_t m1, uint32_t cvec, int idx, uint32_t voff) const {
    if (zs_over(zs_over_bits(m0, m1))) {
      const uint32_t cf = (uint32_t)__builtin_amdgcn_readlane((int)cvec, idx);
      const uint32_t cj = GM == 3 ? (cf & 0x7fffffffu) : cf;
      u2_t d;
      if (GM == 3 && (cf & 0x80000000u))  // (wave-uniform: a cold column's dense row does not allocate either)
        d = __builtin_amdgcn_raw_buffer_load_b64(rsrc2, (int)voff, (int)(cj * ZsTraits<E>::dense_row_bytes), 2);
      else d = __builtin_amdgcn_raw_buffer_load_b64(rsrc2, (int)voff, (int)(cj * ZsTraits<E>::dense_row_bytes), 0);
      typename VecT<VEC>::type v;
      v[0] = __uint_as_float(d[0]);
      v[1] = __uint_as_float(d[1]);
      return v;
    }
    return zs_select(p, m0, m1);
  }
  // zs_select: the zero fill, with the mask itself as lane mask (written out: from `(m >> lane) & 1` the compiler builds a
  // 64-bit shift, two ands and a 64-bit compare per value)
  static __device__ __forceinline__ typename VecT<VEC>::type zs_select(const raw_t& r, zs_mask_t m0, zs_mask_t m1) {
    uint32_t k0, k1;
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(k0) : "v"(r[0]), "s"(m0));
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(k1) : "v"(r[1]), "s"(m1));
    typename VecT<VEC>::type v;
    v[0] = __uint_as_float(k0);
    v[1] = __uint_as_float(k1);
    return v;
  }
  __device__ __forceinline__ typename VecT<VEC>::type load(uint32_t cj, uint32_t voff) const { return widen(load_raw(cj, voff)); }
  __device__ __forceinline__ raw_t load_raw(uint32_t cj, uint32_t voff) const {
    typedef typename VecT<VEC>::type vec_t;
    if constexpr (PART) {
      static_assert(GM == 0 || GM == 1, "two-table gathers: plain buffer or global loads");
      const bool second = cj >= n_first;  // scalar
      if constexpr (GM == 1) {
        const int soff = (int)((second ? cj - n_first : cj) * (uint32_t)ldb);
        return load_rsrc<0>(second ? rsrc2 : rsrc, soff, voff);  // (scalar selects: straight-line code)
      } else {
        const char* rowp = (second ? inb2 : inb) + (int64_t)cj * ldb;
        return *reinterpret_cast<const raw_t*>(rowp + voff);  // (bf16: the packed words, as from the one-table gather)
      }
    } else if constexpr (ZS) {
      // lanes 48 .. 63 ask for offset 0 as out-of-range lanes do: exactly the row's three lines, whatever its header says
      const int zoff = (int)(voff < (uint32_t)GAIB_ZS_ROW_BYTES ? voff : 0u);
      if constexpr (GM == 3) {
        const uint32_t c = cj & 0x7fffffffu;
        if (cj & 0x80000000u) return __builtin_amdgcn_raw_buffer_load_b64(rsrc, zoff, (int)(c * (uint32_t)GAIB_ZS_ROW_BYTES), 2);  // wave-uniform
        return __builtin_amdgcn_raw_buffer_load_b64(rsrc, zoff, (int)(c * (uint32_t)GAIB_ZS_ROW_BYTES), 0);
      } else {
        return __builtin_amdgcn_raw_buffer_load_b64(rsrc, zoff, (int)(cj * (uint32_t)GAIB_ZS_ROW_BYTES), 0);
      }
    } else if constexpr (GM == 3) {
      const uint32_t c = cj & 0x7fffffffu;
      if (cj & 0x80000000u) return load_buf<2>(c, voff);  // wave-uniform branch (cj is scalar)
      return load_buf<0>(c, voff);
    } else if constexpr (GM == 2) {
      return load_buf<2>(cj, voff);
    } else if constexpr (GM == 1) {
      return load_buf<0>(cj, voff);
    } else {
      const char* rowp = inb + (int64_t)cj * ldb;  // scalar base
      if constexpr (sizeof(E) == 2 || F8) return *reinterpret_cast<const raw_t*>(rowp + voff);
      else return *reinterpret_cast<const vec_t*>(rowp + voff);
    }
  }
  template <int AUX>
  __device__ __forceinline__ raw_t load_buf(uint32_t cj, uint32_t voff) const {
    return load_rsrc<AUX>(rsrc, (int)(cj * (uint32_t)ldb), voff);
  }
  template <int AUX>
  __device__ __forceinline__ raw_t load_rsrc(__amdgpu_buffer_rsrc_t rsrc, int soff, uint32_t voff) const {
    typedef typename VecT<VEC>::type vec_t;
    if constexpr (sizeof(E) == 2) {  // bf16: half the bytes per gather (b16 / b32 / b64 / b128 for 1 / 2 / 4 / 8 elements)
      if constexpr (VEC == 1) return __builtin_amdgcn_raw_buffer_load_b16(rsrc, (int)voff, soff, AUX);
      else if constexpr (VEC == 2) return __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, soff, AUX);
      else if constexpr (VEC == 4) return __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)voff, soff, AUX);
      else return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, soff, AUX);
    } else if constexpr (F8) {  // fp8: a quarter of the bytes (b8 / b16 / b32 / b64 for 1 / 2 / 4 / 8 elements)
      if constexpr (VEC == 1) return __builtin_amdgcn_raw_buffer_load_b8(rsrc, (int)voff, soff, AUX);
      else if constexpr (VEC == 2) return __builtin_amdgcn_raw_buffer_load_b16(rsrc, (int)voff, soff, AUX);
      else if constexpr (VEC == 4) return __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, soff, AUX);
      else return __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)voff, soff, AUX);
    } else if constexpr (VEC == 1) {
      return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, soff, AUX));
    } else if constexpr (VEC == 2) {
      u2_t r = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)voff, soff, AUX);
      vec_t v;
      v[0] = __uint_as_float(r[0]);
      v[1] = __uint_as_float(r[1]);
      return v;
    } else {
      u4_t r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, soff, AUX);
      vec_t v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(r[i]);
      return v;
    }
  }
};

// Rows per group of the packed expansion (RowGather::zs_issue / zs_fix / zs_select): the cross-lane reads of a group travel
// together and the group has ONE branch, for the over-capacity path.  A row of a group in flight holds four mask SGPRs, so the
// group size is bounded by the scalar registers: 4 compiles without spilling them in the hot loop, 8 spills (LEDGER 10.4).
#ifndef GAIB_ZS_GROUP
#define GAIB_ZS_GROUP 4
#endif

// G packed rows x[xo .. xo + G - 1] of a batch or of a tail piece -- edges j0 .. j0 + G - 1 of the wave's chunk -- expanded and
// accumulated in CSR order: every product and every addition of the dense loop, in its order.  (The products and sums are
// written on the 2-vector: left to pair them up itself, the compiler pairs the products of two ROWS and shuffles.)
template <int G, int CT, int WMODE, int U, typename gather_t>
__device__ __forceinline__ void zs_accumulate_group(const gather_t& gather, const typename gather_t::raw_t (&x)[U][CT], int xo, uint32_t c, float w,
                                                    float roww, int j0, const uint32_t (&voff)[CT], typename VecT<2>::type (&acc)[CT]) {
  typename gather_t::zs_mask_t m0[G][CT], m1[G][CT];
  typename gather_t::raw_t p[G][CT];
  uint32_t over = 0u;
#pragma unroll
  for (int u = 0; u < G; ++u)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) gather_t::zs_issue(x[xo + u][ct], p[u][ct], m0[u][ct], m1[u][ct], over);
  if (__builtin_expect(gather_t::zs_over(over), 0)) {  // (wave-uniform: the masks are scalars)
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const float wj = (WMODE == 0) ? roww : readlane_f(w, j0 + u);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const typename VecT<2>::type t = gather.zs_fix(p[u][ct], m0[u][ct], m1[u][ct], c, j0 + u, voff[ct]) * wj;
        acc[ct] = acc[ct] + t;
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const float wj = (WMODE == 0) ? roww : readlane_f(w, j0 + u);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const typename VecT<2>::type t = gather_t::zs_select(p[u][ct], m0[u][ct], m1[u][ct]) * wj;
        acc[ct] = acc[ct] + t;
      }
    }
  }
}

// ---- the shared per-wave edge loop: accumulate edges [eb, ee) of one row -------------
// chunk_stride: distance between this wave's 64-edge chunks (64 for a whole row, 64*W when
// W waves share a row).
// voff[ct] is the lane's BYTE offset inside a feature row; lanes whose columns fall outside
// the row are pointed at offset 0, so every gather is unconditional (a predicated load makes
// hipcc branch on EXEC and drain vmcnt after each one); what they accumulate is never stored.
// PRE: the column ids (and weights) of the row's FIRST chunk were requested by the caller ahead of time (c_first / w_first,
// lane l = edge eb + l, 0 past the row's end) -- the fused kernel asks for row r + 1's while row r's gathers are in flight.
template <int VEC, int CT, int WMODE, int U, int BUF, bool PART = false, bool PRE = false, typename E = float>
__device__ __forceinline__ void wave_accumulate(const SpmmArgs& a, int lane, int64_t eb, int64_t ee,
                                                int64_t chunk_stride, float roww,
                                                const uint32_t (&voff)[CT],
                                                typename VecT<VEC>::type (&acc)[CT], uint32_t c_first = 0u,
                                                float w_first = 0.f) {
  static_assert((sizeof(E) == 4 && !ZsTraits<E>::zs) || WMODE < 3, "bf16 and zero-suppressed tables: single-head weights");
  typedef RowGather<VEC, BUF, PART, E> gather_t;
  const gather_t gather(a);
  typename gather_t::raw_t x[U][CT];  // gather destinations (bf16: packed words, widened where consumed); the tail's piece p lives in x[p .. 2p-1]
  constexpr bool MH = WMODE >= 3;  // multi-head: every lane fetches the weight of ITS head itself
  // fp8 tables: lane l's weight is w_e * scale[col_e] in every single-head mode (WMODE 0: roww * scale[col_e], so that mode
  // reads its weight through the readlane too)
  constexpr bool F8 = gather_t::F8;
  static_assert(!F8 || !PRE, "fp8 tables: the caller's prefetched weights do not carry the scales");
  constexpr bool LANE_W = WMODE != 0 || F8;  // the edge's weight comes from lane j of w (else: roww)
  int hd[CT];
  float wv[MH ? U : 1][CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    // the head of the lane's column IN THE WHOLE ROW: voff counts from the launch's first column, a.col0 (lanes outside
    // the row sit at offset 0, whose head col0 / dh is a valid one)
    if constexpr (MH) hd[ct] = (int)(((uint32_t)a.col0 + (voff[ct] >> 2)) / (uint32_t)a.dh);
    else hd[ct] = 0;
  }
  for (int64_t base = eb; base < ee; base += chunk_stride) {
    const int64_t rem = ee - base;
    const int n = rem < 64 ? (int)rem : 64;  // wave-uniform
    uint32_t c = 0;
    float w = 0.f;
    if (PRE && base == eb) {  // (wave-uniform)
      c = c_first;
      w = w_first;
    } else if (lane < n) {
      c = a.col[base + lane];
      if constexpr (WMODE == 1 || WMODE == 2) w = load_edge_w<WMODE>(a, base + lane);
      if constexpr (F8) w = fp8_fold_scale<BUF>(a, c, WMODE == 0 ? roww : w);
    }
    int j = 0;
    // full batches: U independent row gathers in flight, straight-line code
    for (; j + U <= n; j += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)c, j + u);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          x[u][ct] = gather.load_raw(cj, voff[ct]);
          if constexpr (MH) wv[u][ct] = load_edge_w<WMODE>(a, base + j + u, hd[ct]);
        }
      }
      // all U gathers are issued before the first one is consumed: without the fence the scheduler may interleave
      // loads and uses to save registers (seen in the two-product fused kernel: vmcnt(1) after every load)
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (gather_t::ZS) {
        constexpr int H = GAIB_ZS_GROUP < U ? GAIB_ZS_GROUP : U;
#pragma unroll
        for (int u = 0; u < U; u += H) zs_accumulate_group<H, CT, WMODE>(gather, x, u, c, w, roww, j + u, voff, acc);
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float wj = !LANE_W ? roww : (MH ? 0.f : readlane_f(w, j + u));
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            float wsel = wj;
            if constexpr (MH) wsel = wv[u][ct];
            vacc<VEC>(acc[ct], wsel, gather_t::widen(x[u][ct]));
          }
        }
      }
    }
    // tail: r = n - j < U edges, done as power-of-two pieces U/2, U/4, .., 1 (CSR order kept):
    // first every piece's gathers are issued, then every piece is accumulated.
    const int r = n - j;
    if (r > 0) {
      int jj = j;
#pragma unroll
      for (int p = U / 2; p >= 1; p >>= 1) {
        if (r & p) {
#pragma unroll
          for (int u = 0; u < p; ++u) {
            const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)c, jj + u);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) x[p + u][ct] = gather.load_raw(cj, voff[ct]);
          }
          jj += p;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      jj = j;
#pragma unroll
      for (int p = U / 2; p >= 1; p >>= 1) {
        if (r & p) {
          if constexpr (gather_t::ZS) {  // a piece is one group, or whole groups
            if (p >= GAIB_ZS_GROUP) {
#pragma unroll
              for (int u = 0; u < p; u += GAIB_ZS_GROUP)
                zs_accumulate_group<GAIB_ZS_GROUP, CT, WMODE>(gather, x, p + u, c, w, roww, jj + u, voff, acc);
            } else if (p == 8) zs_accumulate_group<8, CT, WMODE>(gather, x, p, c, w, roww, jj, voff, acc);
            else if (p == 4) zs_accumulate_group<4, CT, WMODE>(gather, x, p, c, w, roww, jj, voff, acc);
            else if (p == 2) zs_accumulate_group<2, CT, WMODE>(gather, x, p, c, w, roww, jj, voff, acc);
            else zs_accumulate_group<1, CT, WMODE>(gather, x, p, c, w, roww, jj, voff, acc);
          } else {
#pragma unroll
            for (int u = 0; u < p; ++u) {
              const float wj = !LANE_W ? roww : (MH ? 0.f : readlane_f(w, jj + u));
#pragma unroll
              for (int ct = 0; ct < CT; ++ct) {
                // (the tail is short: its per-head weights are fetched at the point of use)
                float wh = wj;
                if constexpr (MH) wh = load_edge_w<WMODE>(a, base + jj + u, hd[ct]);
                vacc<VEC>(acc[ct], wh, gather_t::widen(x[p + u][ct]));
              }
            }
          }
          jj += p;
        }
      }
    }
  }
}

}  // namespace
