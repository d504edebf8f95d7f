// split_planes.h -- what sgemm_split.hip and sgemm_split_tn.hip share: an fp32 value as the exact sum of three truncated bf16
// planes, eight values at a time in the register layout of one v_mfma_f32_16x16x32_bf16 operand.
#pragma once
#include "common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf8_t __attribute__((ext_vector_type(8)));

constexpr int SS_OUTSIDE = 0x7ffffff0;  // a byte offset outside every descriptor (at most 2^30 bytes): reads 0, store dropped

__device__ __forceinline__ f4 ss_mfma(u4_t a, u4_t b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8_t, a), __builtin_bit_cast(bf8_t, b), c, 0, 0, 0);
}

// 8 consecutive fp32 values of a row -> their three truncated bf16 planes, packed (element e in half e & 1 of register e >> 1)
__device__ __forceinline__ void ss_split8(const u4_t lo, const u4_t hi, u4_t (&p)[3]) {
  unsigned a[8], r1[8], r2[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = lo[e];
    a[4 + e] = hi[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    r1[e] = __float_as_uint(__uint_as_float(a[e]) - __uint_as_float(a[e] & 0xffff0000u));
    r2[e] = __float_as_uint(__uint_as_float(r1[e]) - __uint_as_float(r1[e] & 0xffff0000u));
  }
#pragma unroll
  for (int h = 0; h < 4; ++h) {  // (high half of the odd element | high half of the even one >> 16)
    p[0][h] = __builtin_amdgcn_perm(a[2 * h + 1], a[2 * h], 0x07060302u);
    p[1][h] = __builtin_amdgcn_perm(r1[2 * h + 1], r1[2 * h], 0x07060302u);
    p[2][h] = __builtin_amdgcn_perm(r2[2 * h + 1], r2[2 * h], 0x07060302u);
  }
}

}  // namespace
