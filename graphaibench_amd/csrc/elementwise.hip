// elementwise.hip -- relu / dropout / loss / l2norm / adam / row gather for gfx950.
// All of these are HBM-streaming: 16 B per lane, grid capped at 2048 workgroups with a
// grid-stride loop (cdna guide, Guideline 11/13).
//
// replaces relu_gpu / d_relu_gpu / dropout_gpu / d_dropout_gpu / init_const_gpu /
// softmax_cross_entropy_gpu / d_softmax_cross_entropy_gpu / masked_avg_loss_gpu /
// masked_accuracy_single / l2norm / d_l2norm (src/utilities/math_functions.cu:12-14,
// 114-146, 158-196, 242-268, 516-564, 749-761, 886-942) and adam::update_gpu
// (src/utilities/optimizer.cu:5-36).
#include <algorithm>
#include "common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

inline unsigned stream_grid(int64_t n_items, int block) {
  int64_t b = cdiv64(n_items > 0 ? n_items : 1, block);
  return (unsigned)(b < 2048 ? b : 2048);
}

__global__ void fill_kernel(int64_t n, float v, float* x) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = v;
}

__global__ void scale_kernel(int64_t n, float a, float* x) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = a * x[i];
}

// relu_cpu / relu_kernel: max(x, 0)    (math_functions.cpp:442-451; .cu:242)
__global__ void relu_kernel(int64_t n, const float* in, float* out, int vec_ok) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec_ok) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += stride) {
      f4 v = reinterpret_cast<const f4*>(in)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
      reinterpret_cast<f4*>(out)[i] = v;
    }
    for (int64_t i = (n4 << 2) + tid; i < n; i += stride) out[i] = in[i] > 0.f ? in[i] : 0.f;
  } else {
    for (int64_t i = tid; i < n; i += stride) out[i] = in[i] > 0.f ? in[i] : 0.f;
  }
}

// d_relu: out = data > 0 ? in : 0     (math_functions.cpp:453-463; .cu:255)
__global__ void d_relu_kernel(int64_t n, const float* in, const float* data, float* out, int vec_ok) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec_ok) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += stride) {
      f4 g = reinterpret_cast<const f4*>(in)[i];
      f4 d = reinterpret_cast<const f4*>(data)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] = d[k] > 0.f ? g[k] : 0.f;
      reinterpret_cast<f4*>(out)[i] = g;
    }
    for (int64_t i = (n4 << 2) + tid; i < n; i += stride) out[i] = data[i] > 0.f ? in[i] : 0.f;
  } else {
    for (int64_t i = tid; i < n; i += stride) out[i] = data[i] > 0.f ? in[i] : 0.f;
  }
}

// dropout_kernel (u01: common.h): mask = rand > p; out = in * mask * scale   (math_functions.cu:114-121)
__global__ void dropout_kernel(int64_t n, float scale, float rate, uint64_t seed, const float* in,
                               uint8_t* masks, float* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint8_t m = u01(seed, (uint64_t)i) > rate ? 1 : 0;
    masks[i] = m;
    out[i] = in[i] * (float)m * scale;
  }
}
// The same draw with the seed in device memory (*seed_p): a recorded (HIP graph) dropout cannot take it by value.  16-B lanes:
// a thread owns 4 consecutive elements (one 16-B load, one 16-B store, the 4 mask bytes as one 4-B store).  u01_key is linear in
// the index, so element e + 1's key is element e's plus U01_GOLD, and the next trip's is this trip's plus U01_GOLD * 4 * stride:
// one 64-bit add per element where dropout_kernel multiplies.  Same value expression, same bits.  vec_ok == 0 (pointers not
// 16 / 16 / 4-B aligned) and the n % 4 tail take the scalar form.  seed_advance_kernel is the host's `seed++`.
__global__ __launch_bounds__(256) void dropout_dev_kernel(int64_t n, float scale, float rate, const uint64_t* seed_p,
                                                          const float* in, uint8_t* masks, float* out, int vec_ok) {
  const uint64_t seed = *seed_p;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t tail0 = 0;
  if (vec_ok) {
    const int64_t n4 = n >> 2;
    uint64_t key = u01_key(seed, (uint64_t)tid << 2);
    const uint64_t key_step = U01_GOLD * ((uint64_t)stride << 2);
    for (int64_t i = tid; i < n4; i += stride, key += key_step) {
      f4 v = reinterpret_cast<const f4*>(in)[i];
      uint32_t mw = 0;
      uint64_t k64 = key;
#pragma unroll
      for (int k = 0; k < 4; ++k, k64 += U01_GOLD) {
        const uint8_t m = u01_of_key(k64) > rate ? 1 : 0;
        mw |= (uint32_t)m << (8 * k);
        v[k] = v[k] * (float)m * scale;
      }
      reinterpret_cast<f4*>(out)[i] = v;
      reinterpret_cast<uint32_t*>(masks)[i] = mw;
    }
    tail0 = n4 << 2;
  }
  for (int64_t i = tail0 + tid; i < n; i += stride) {
    const uint8_t m = u01(seed, (uint64_t)i) > rate ? 1 : 0;
    masks[i] = m;
    out[i] = in[i] * (float)m * scale;
  }
}
__global__ void seed_advance_kernel(uint64_t* seed_p) { seed_p[0] += 1; }

__global__ void d_dropout_kernel(int64_t n, float scale, const float* in, const uint8_t* masks,
                                 float* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = in[i] * (float)masks[i] * scale;
}

// softmax + cross entropy per vertex (softmax_loss_layer.cpp:4-21; math_functions.cpp:485-494,
// 533-544).  One wave per vertex, classes across lanes (num_cls is small: 7..172).
__global__ __launch_bounds__(256) void softmax_xent_kernel(int num_cls, int64_t begin, int64_t end,
                                                           const float* in, const uint8_t* masks,
                                                           const uint8_t* labels, float* loss,
                                                           float* out) {
  const int64_t i = begin + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= end) return;
  if (masks && masks[i] != 1) return;
  const int lane = threadIdx.x & 63;
  const float* x = in + i * (int64_t)num_cls;
  float* y = out + i * (int64_t)num_cls;
  float mx = -INFINITY;
  for (int c = lane; c < num_cls; c += 64) mx = fmaxf(mx, x[c]);
  mx = wave_max(mx);
  float den = 0.f;
  for (int c = lane; c < num_cls; c += 64) den += expf(x[c] - mx);
  den = wave_sum(den);
  const int lab = labels[i];
  float pl = 0.f;
  for (int c = lane; c < num_cls; c += 64) {
    const float p = expf(x[c] - mx) / den;
    y[c] = p;
    if (c == lab) pl = p;
  }
  pl = wave_sum(pl);  // exactly one lane holds it
  if (lane == 0) loss[i] = (pl == 0.0f) ? -logf(1e-10f) : -logf(pl);
}

// (p - onehot) / (end - begin)   (softmax_loss_layer.cpp:23-37, Q8)
__global__ void d_softmax_xent_kernel(int num_cls, int64_t begin, int64_t end,
                                      const uint8_t* masks, const uint8_t* labels,
                                      const float* out, float* diff) {
  const int64_t n = (end - begin) * num_cls;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const double inv = (double)(end - begin);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
    const int64_t i = begin + t / num_cls;
    const int j = (int)(t % num_cls);
    if (masks && masks[i] != 1) continue;
    const float pred = out[i * num_cls + j];
    diff[i * num_cls + j] = (float)(((double)pred - (labels[i] == j ? 1.0 : 0.0)) / inv);
  }
}

// sigmoid + cross entropy per vertex for multi-label heads (sigmoid_loss_layer.cpp:4-17,
// math_functions.cpp:517-521,553-559): labels are [n x num_cls] 0/1 bytes.  One wave per
// vertex, classes across lanes; masked-out vertices of the range get loss 0 (the .cu layer
// zeroes d_losses first, sigmoid_loss_layer.cu:6).
__global__ __launch_bounds__(256) void sigmoid_xent_kernel(int num_cls, int64_t begin, int64_t end,
                                                           const float* in, const uint8_t* masks,
                                                           const uint8_t* labels, float* loss,
                                                           float* out) {
  const int64_t i = begin + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= end) return;
  const int lane = threadIdx.x & 63;
  if (masks && masks[i] != 1) {
    if (lane == 0) loss[i] = 0.f;
    return;
  }
  const float* x = in + i * (int64_t)num_cls;
  const uint8_t* y = labels + i * (int64_t)num_cls;
  float* o = out + i * (int64_t)num_cls;
  float part = 0.f;
  for (int c = lane; c < num_cls; c += 64) {
    const float p = x[c];
    o[c] = (float)(1. / (1. + (double)expf(-p)));
    const float pos = p >= 0.f ? 1.f : 0.f;
    const float e = expf((float)((double)p - 2. * (double)p * (double)pos));
    part -= p * ((float)y[c] - pos) - logf((float)(1. + (double)e));
  }
  part = wave_sum(part);
  if (lane == 0) loss[i] = part;
}

// (sigmoid - label) / (end - begin)   (sigmoid_loss_layer.cpp:19-33)
__global__ void d_sigmoid_xent_kernel(int num_cls, int64_t begin, int64_t end,
                                      const uint8_t* masks, const uint8_t* labels,
                                      const float* out, float* diff) {
  const int64_t n = (end - begin) * num_cls;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float inv = (float)(uint64_t)(end - begin);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
    const int64_t i = begin + t / num_cls;
    if (masks && masks[i] != 1) continue;
    const int64_t idx = begin * num_cls + t;
    diff[idx] = (out[idx] - (float)labels[idx]) / inv;
  }
}

// tp / fp / fn over every (vertex, class) cell of the masked range (math_functions.cpp:580-603):
// integer counts, so the atomics are order-independent.
__global__ __launch_bounds__(256) void f1_counts_kernel(int num_cls, int64_t begin, int64_t end,
                                                        const uint8_t* masks, const float* preds,
                                                        const uint8_t* labels,
                                                        unsigned long long* counts) {
  const int64_t n = (end - begin) * num_cls;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned tp = 0, fp = 0, fn = 0;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
    const int64_t i = begin + t / num_cls;
    if (masks && masks[i] != 1) continue;
    const int64_t idx = begin * num_cls + t;
    const bool hot = preds[idx] > 0.5f;
    const uint8_t y = labels[idx];
    tp += (y == 1 && hot);
    fp += (y == 0 && hot);
    fn += (y == 1 && preds[idx] <= 0.5f);  // (not `!hot`: a NaN prediction is neither, math_functions.cpp:596)
  }
  __shared__ unsigned s[3];
  if (threadIdx.x < 3) s[threadIdx.x] = 0;
  __syncthreads();
  tp = (unsigned)wave_sum_u32(tp);
  fp = (unsigned)wave_sum_u32(fp);
  fn = (unsigned)wave_sum_u32(fn);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&s[0], tp);
    atomicAdd(&s[1], fp);
    atomicAdd(&s[2], fn);
  }
  __syncthreads();
  if (threadIdx.x < 3 && s[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s[threadIdx.x]);
}

// two-level deterministic masked reductions ------------------------------------------------
// partial[b] = {sum, count} over a strip; final sum over b in order on the host side of the
// C ABI (nblocks <= 1024 values).
__global__ __launch_bounds__(256) void masked_loss_partial_kernel(int64_t begin, int64_t end,
                                                                  const uint8_t* masks,
                                                                  const float* loss, float* part) {
  __shared__ float ssum[4], scnt[4];
  float s = 0.f, c = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride)
    if (!masks || masks[i] == 1) {
      s += loss[i];
      c += 1.f;
    }
  s = wave_sum(s);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) {
    ssum[threadIdx.x >> 6] = s;
    scnt[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = ssum[0] + ssum[1] + ssum[2] + ssum[3];
    part[2 * blockIdx.x + 1] = scnt[0] + scnt[1] + scnt[2] + scnt[3];
  }
}

// argmax (first maximum, math_functions.cpp:127-137) == label ?   one thread per vertex
__global__ __launch_bounds__(256) void masked_acc_partial_kernel(int64_t begin, int64_t end,
                                                                 int num_cls, const uint8_t* masks,
                                                                 const float* preds,
                                                                 const uint8_t* labels, float* part) {
  __shared__ float ssum[4], scnt[4];
  float s = 0.f, c = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride)
    if (!masks || masks[i] == 1) {
      const float* p = preds + i * (int64_t)num_cls;
      int best = -1;
      float mx = -INFINITY;
      for (int j = 0; j < num_cls; ++j)
        if (p[j] > mx) {
          mx = p[j];
          best = j;
        }
      if (best == (int)labels[i]) s += 1.f;
      c += 1.f;
    }
  s = wave_sum(s);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) {
    ssum[threadIdx.x >> 6] = s;
    scnt[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = ssum[0] + ssum[1] + ssum[2] + ssum[3];
    part[2 * blockIdx.x + 1] = scnt[0] + scnt[1] + scnt[2] + scnt[3];
  }
}

// l2norm_layer forward/backward (src/layers/l2norm_layer.cpp:19-64), one wave per row
__global__ __launch_bounds__(256) void l2norm_kernel(int64_t n, int dim, const float* in, float* out) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const float* x = in + i * (int64_t)dim;
  float s = 0.f;
  for (int c = lane; c < dim; c += 64) s += x[c] * x[c];
  s = wave_sum(s);
  s = s < 1.0e-12f ? 1.0e-12f : s;
  s = sqrtf(s);
  for (int c = lane; c < dim; c += 64) out[i * (int64_t)dim + c] = x[c] / s;
}
__global__ __launch_bounds__(256) void d_l2norm_kernel(int64_t n, int dim, const float* fin,
                                                       const float* gin, float* gout) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const float* x = fin + i * (int64_t)dim;
  const float* g = gin + i * (int64_t)dim;
  float s2 = 0.f, c0 = 0.f;
  for (int c = lane; c < dim; c += 64) {
    s2 += x[c] * x[c];
    c0 -= x[c] * g[c];
  }
  s2 = wave_sum(s2);
  c0 = wave_sum(c0);
  s2 = s2 < 1.0e-12f ? 1.0e-12f : s2;
  if (s2 > 1.0e25f) {
    // s2^-1.5 is below the smallest normal fp32 from 1.9e25 on and below the smallest subnormal from 8e29 on: the row's
    // gradient (about g / |x|, an ordinary number) came out as 0.  The same expression with the coefficient in two factors.
    const float rs = 1.0f / sqrtf(s2), q = c0 / s2;
    for (int c = lane; c < dim; c += 64) gout[i * (int64_t)dim + c] = (x[c] * q + g[c]) * rs;
    return;
  }
  const float c1 = powf(s2, -1.5f);
  for (int c = lane; c < dim; c += 64)
    gout[i * (int64_t)dim + c] = x[c] * c0 * c1 + g[c] * s2 * c1;
}

// adam::update (src/utilities/optimizer.cpp:22-35; update_kernel optimizer.cu:5-15):
// eps inside the sqrt; the caller advances b1_t/b2_t once per call.
__global__ void adam_kernel(int64_t n, const float* dW, float* W, float* m, float* v, float alpha,
                            float b1, float b2, float b1_t, float b2_t, float eps) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float g = dW[i];
    const float mt = b1 * m[i] + (1.0f - b1) * g;
    const float vt = b2 * v[i] + (1.0f - b2) * g * g;
    m[i] = mt;
    v[i] = vt;
    W[i] -= alpha * (mt / (1.0f - b1_t)) / sqrtf((vt / (1.0f - b2_t)) + eps);
  }
}

// out[k,:] = in[idx[k],:]   (halo send-buffer packing).
// 16-B path: a wave copies GR_ROWS consecutive output rows, i.e. one contiguous piece of `out`; lane l of step u moves
// float4 number u*64 + l of that piece, so stores are whole 1-KB wave writes and GR_U row pieces are in flight per
// wave before the first store (one row per wave left every wave with a single dependent load: 4.0 TB/s read+write at
// 6.4 M rows of 512 B).  The source row of a piece comes from the wave's 16 row ids, held one per lane.
constexpr int GR_ROWS = 16;
constexpr int GR_U = 8;
// SCATTER: out[didx[k],:] = in[idx[k],:] -- the pack of a halo plan in SOURCE order (idx ascending, the same row up to
// once per peer back to back): a row that goes to several peers is read from HBM once and found in the cache by its
// repeats, where the destination-ordered pack read it once per peer (2.6 x at 8 ranks); the 512-B row pieces land in
// their (scattered) slots of the send buffer.
// SCATTER == 2: didx[k] is the ADDRESS of destination row k (a send buffer cut into separately allocated chunks: comm.hip)
template <int SCATTER>
__global__ __launch_bounds__(256) void gather_rows_vec_kernel(int64_t n_idx, const int64_t* idx, const int64_t* didx, int n4,
                                                              int shift, const f4* in, f4* out) {
  const int lane = threadIdx.x & 63;
  const int64_t k0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * GR_ROWS;
  if (k0 >= n_idx) return;
  const int rows = (n_idx - k0 < GR_ROWS) ? (int)(n_idx - k0) : GR_ROWS;
  const int64_t mine = idx[k0 + (lane < rows ? lane : rows - 1)];
  const int mine_lo = (int)(uint32_t)(mine & 0xffffffffll), mine_hi = (int)(mine >> 32);
  int dst_lo = 0, dst_hi = 0;
  if constexpr (SCATTER != 0) {
    const int64_t d = didx[k0 + (lane < rows ? lane : rows - 1)];
    dst_lo = (int)(uint32_t)(d & 0xffffffffll);
    dst_hi = (int)(d >> 32);
  }
  const int items = rows * n4;
  f4* dst = out + k0 * n4;
  for (int t0 = 0; t0 < items; t0 += 64 * GR_U) {
    f4 v[GR_U];
#pragma unroll
    for (int u = 0; u < GR_U; ++u) {
      int t = t0 + u * 64 + lane;
      if (t >= items) t = items - 1;  // clamped: every lane loads, only real items are stored
      const int r = shift >= 0 ? (t >> shift) : (t / n4);
      const int c = t - r * n4;
      const int64_t src = ((int64_t)__shfl(mine_hi, r) << 32) | (uint32_t)__shfl(mine_lo, r);
      v[u] = in[src * n4 + c];
    }
#pragma unroll
    for (int u = 0; u < GR_U; ++u) {
      const int t = t0 + u * 64 + lane;
      if constexpr (SCATTER != 0) {
        const int tc = t < items ? t : items - 1;
        const int r = shift >= 0 ? (tc >> shift) : (tc / n4);
        const int c = tc - r * n4;
        const int64_t drow = ((int64_t)__shfl(dst_hi, r) << 32) | (uint32_t)__shfl(dst_lo, r);
        if constexpr (SCATTER == 2) {
          if (t < items) reinterpret_cast<f4*>(drow)[c] = v[u];
        } else {
          if (t < items) out[drow * n4 + c] = v[u];
        }
      } else {
        if (t < items) dst[t] = v[u];
      }
    }
  }
}

// 4-B path (row length not a multiple of 4 floats, or unaligned tables): one wave per row
__global__ __launch_bounds__(256) void gather_rows_kernel(int64_t n_idx, const int64_t* idx, int len,
                                                          const float* in, float* out) {
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n_idx) return;
  const int lane = threadIdx.x & 63;
  const float* src = in + idx[k] * (int64_t)len;
  float* dst = out + k * (int64_t)len;
  for (int c = lane; c < len; c += 64) dst[c] = src[c];
}

__global__ __launch_bounds__(256) void scatter_rows_kernel(int64_t n_idx, const int64_t* idx, const int64_t* didx, int len,
                                                           const float* in, float* out) {
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n_idx) return;
  const int lane = threadIdx.x & 63;
  const float* src = in + idx[k] * (int64_t)len;
  float* dst = out + didx[k] * (int64_t)len;
  for (int c = lane; c < len; c += 64) dst[c] = src[c];
}

int finish_partial(gaib_ctx* ctx, int nblocks, float* d_part, float* h_result) {
  GAIB_NOT_WHILE_CAPTURING(ctx, "a metric with a host result (use the *_dev form)");
  float h[2 * 1024];
  GAIB_HIP(hipMemcpyAsync(h, d_part, sizeof(float) * 2 * nblocks, hipMemcpyDeviceToHost, ctx->stream));
  GAIB_HIP(hipStreamSynchronize(ctx->stream));
  float s = 0.f, c = 0.f;
  for (int b = 0; b < nblocks; ++b) {
    s += h[2 * b];
    c += h[2 * b + 1];
  }
  *h_result = c > 0.f ? s / c : 0.f;
  return GAIB_OK;
}

// the device-side twin of finish_partial: the block partials are added in block order by ONE thread (the host loop's
// order and roundings), result[0] = sum / count
__global__ void finish_partial_kernel(int nblocks, const float* part, float* result) {
  __shared__ float sh[2 * 1024];
  for (int t = threadIdx.x; t < 2 * nblocks; t += blockDim.x) sh[t] = part[t];
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f, c = 0.f;
    for (int b = 0; b < nblocks; ++b) {
      s += sh[2 * b];
      c += sh[2 * b + 1];
    }
    result[0] = c > 0.f ? s / c : 0.f;
  }
}

// bias_mv (math_functions.cu:207-221): x[i, j] += b[j]
__global__ void bias_add_kernel(int64_t total, int len, float* x, const float* b) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) x[i] = x[i] + b[i % len];
}
// reduce_sum (math_functions.cpp:246-262: a[j] = sum_i x[i, j]; the reference's CUDA kernel, math_functions.cu:224-229,
// adds into a[j] from every thread without atomics).  Two levels in a fixed order: block b sums its run of rows per
// column, then the block partials are added in block order -- the same bits on every run.
__global__ __launch_bounds__(256) void colsum_partial_kernel(int64_t n, int len, int64_t rows_per_block, const float* x,
                                                             float* part) {
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  for (int j = threadIdx.x; j < len; j += blockDim.x) {
    float s = 0.f;
    for (int64_t i = r0; i < r1; ++i) s += x[i * len + j];
    part[(int64_t)blockIdx.x * len + j] = s;
  }
}
__global__ void colsum_finish_kernel(int nblocks, int len, const float* part, float* a) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= len) return;
  float s = 0.f;
  for (int b = 0; b < nblocks; ++b) s += part[(int64_t)b * len + j];
  a[j] = s;
}
// rng_uniform_gpu / gpu_rng_uniform (math_functions.cu:39-50): r = a + (b - a) * u, u uniform on [0, 1) from the
// library's counter RNG (the reference draws cuRAND XORWOW numbers: streams are not comparable, statistics are)
__global__ void rng_uniform_kernel(int64_t n, float a, float range, uint64_t seed, float* r) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) r[i] = a + range * u01(seed, (uint64_t)i);
}

// Adam with the beta powers in device memory (pw[0] = b1^t, pw[1] = b2^t): a recorded (HIP graph) step cannot take
// them by value.  adam_advance_kernel is the host's `b1_t *= b1; b2_t *= b2` (optimizer.cpp), same float products.
__global__ void adam_dev_kernel(int64_t n, const float* dW, float* W, float* m, float* v, float alpha, float b1,
                                float b2, const float* pw, float eps) {
  const float b1_t = pw[0], b2_t = pw[1];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float g = dW[i];
    const float mt = b1 * m[i] + (1.0f - b1) * g;
    const float vt = b2 * v[i] + (1.0f - b2) * g * g;
    m[i] = mt;
    v[i] = vt;
    W[i] -= alpha * (mt / (1.0f - b1_t)) / sqrtf((vt / (1.0f - b2_t)) + eps);
  }
}
__global__ void adam_advance_kernel(float* pw, float b1, float b2) {
  pw[0] *= b1;
  pw[1] *= b2;
}

// ---- bf16 feature tables: f32 <-> bf16 (raw bits in uint16_t) -----------------------------------------------------
// f32 -> bf16 rounds to nearest, ties to even, on the bit pattern (what torch's CPU .to(torch.bfloat16) does): subnormals
// are kept, finite values past the largest bf16 round up to +-inf, +-inf stay.  A NaN stays a NaN of the same sign: its
// upper half with the quiet bit set (a NaN whose payload sits in the low half alone must not become inf).
// bf16 -> f32 is exact: bits << 16.
__device__ __forceinline__ unsigned f32_to_bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
typedef unsigned u4v __attribute__((ext_vector_type(4)));
// one thread per 8 elements: two 16-B loads, one 16-B store (vec: both pointers 16-B aligned); the n % 8 tail by the
// thread of group n / 8
__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(int64_t n, const float* __restrict__ in, uint16_t* __restrict__ out,
                                                            int vec) {
  const int64_t n8 = vec ? n / 8 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n8; i += stride) {
    if (i < n8) {
      const f4 a = reinterpret_cast<const f4*>(in)[2 * i], b = reinterpret_cast<const f4*>(in)[2 * i + 1];
      u4v o;
      o[0] = f32_to_bf16_bits(a[0]) | (f32_to_bf16_bits(a[1]) << 16);
      o[1] = f32_to_bf16_bits(a[2]) | (f32_to_bf16_bits(a[3]) << 16);
      o[2] = f32_to_bf16_bits(b[0]) | (f32_to_bf16_bits(b[1]) << 16);
      o[3] = f32_to_bf16_bits(b[2]) | (f32_to_bf16_bits(b[3]) << 16);
      reinterpret_cast<u4v*>(out)[i] = o;
    } else {
      for (int64_t k = 8 * n8; k < n; ++k) out[k] = (uint16_t)f32_to_bf16_bits(in[k]);
    }
  }
}
// scalar form (unaligned pointers): one element per thread
__global__ __launch_bounds__(256) void cast_f32_bf16_scalar_kernel(int64_t n, const float* __restrict__ in,
                                                                   uint16_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (uint16_t)f32_to_bf16_bits(in[i]);
}
// rows of `len` floats -> rows of `ld` bf16 elements (ld >= len), the columns behind len written as +0.0: the table a strided
// gather reads (gaib_spmm_bf16_ld), made in the one pass the cast is anyway.  One thread per 8 output elements (ld % 8 == 0,
// out 16-B aligned): one 16-B store; the load side reads the thread's 8 floats as two 16-B loads where the input row allows
// (in 16-B aligned, len % 4 == 0), else float by float (a 47-float row starts on any 4-B boundary).
template <bool VIN>
__global__ __launch_bounds__(256) void cast_f32_bf16_rows_kernel(int64_t n8, int len, int ld8, const float* __restrict__ in,
                                                                 uint16_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    const int64_t r = i / ld8;
    const int c = (int)(i - r * ld8) * 8;
    const float* src = in + r * len + c;
    float v[8];
    if (VIN && c + 8 <= len) {
      const f4 a = reinterpret_cast<const f4*>(src)[0], b = reinterpret_cast<const f4*>(src)[1];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = a[k], v[4 + k] = b[k];
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = c + k < len ? src[k] : 0.f;
    }
    u4v o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned lo = c + 2 * k < len ? f32_to_bf16_bits(v[2 * k]) : 0u;  // (a pad column is +0.0 whatever sign a 0.f would round to)
      const unsigned hi = c + 2 * k + 1 < len ? f32_to_bf16_bits(v[2 * k + 1]) : 0u;
      o[k] = lo | (hi << 16);
    }
    reinterpret_cast<u4v*>(out)[i] = o;
  }
}
// element-wise form (ld % 8 != 0 or a misaligned output): one output element per thread
__global__ __launch_bounds__(256) void cast_f32_bf16_rows_scalar_kernel(int64_t n, int len, int64_t ld, const float* __restrict__ in,
                                                                        uint16_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t r = i / ld;
    const int64_t c = i - r * ld;
    out[i] = c < len ? (uint16_t)f32_to_bf16_bits(in[r * len + c]) : (uint16_t)0;
  }
}
__global__ __launch_bounds__(256) void cast_bf16_f32_scalar_kernel(int64_t n, const uint16_t* __restrict__ in,
                                                                   float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = __uint_as_float((unsigned)in[i] << 16);
}
// one thread per 8 elements: one 16-B load, two 16-B stores (vec: both pointers 16-B aligned)
__global__ __launch_bounds__(256) void cast_bf16_f32_kernel(int64_t n, const uint16_t* __restrict__ in, float* __restrict__ out,
                                                            int vec) {
  const int64_t n8 = vec ? n / 8 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n8; i += stride) {
    if (i < n8) {
      const u4v w = reinterpret_cast<const u4v*>(in)[i];
      f4 a, b;
      a[0] = __uint_as_float(w[0] << 16);
      a[1] = __uint_as_float(w[0] & 0xffff0000u);
      a[2] = __uint_as_float(w[1] << 16);
      a[3] = __uint_as_float(w[1] & 0xffff0000u);
      b[0] = __uint_as_float(w[2] << 16);
      b[1] = __uint_as_float(w[2] & 0xffff0000u);
      b[2] = __uint_as_float(w[3] << 16);
      b[3] = __uint_as_float(w[3] & 0xffff0000u);
      reinterpret_cast<f4*>(out)[2 * i] = a;
      reinterpret_cast<f4*>(out)[2 * i + 1] = b;
    } else {
      for (int64_t k = 8 * n8; k < n; ++k) out[k] = __uint_as_float((unsigned)in[k] << 16);
    }
  }
}

// ---- zero-suppressed tables (the gather side is RowGather<.., zs_t>, spmm_core.h) -----------------------------------------
// A row of 128 floats -> 96 dwords on a 128-B boundary: M0 (bit l: column 2l holds anything but bit pattern 0), M1 (column 2l + 1),
// then pairs: dword 4 + 2k is the k-th kept value of the even columns, dword 5 + 2k the k-th of the odd columns (as bits, in lane
// order); the rest of the row is 0.  Only bit pattern 0x00000000 is suppressed (-0.0, NaN, inf and subnormals are values), so
// unpacking reproduces the table bit for bit.  A row with more than ZS_CAP values in either half keeps its masks only: its
// consumer reads the dense row.
// One wave per row: one 8-B load per lane, two ballots, mbcnt positions; the row is put together in the wave's 384 B of LDS
// (a wave's LDS operations complete in order) and leaves as one coalesced non-temporal store of three whole lines.
constexpr int ZS_ROW_DW = 96;
constexpr int ZS_CAP = 46;
typedef unsigned zs_u2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void pack_zs_kernel(int64_t rows, const float* __restrict__ in, unsigned* __restrict__ out,
                                                       unsigned* __restrict__ overflow) {
  __shared__ __attribute__((aligned(16))) unsigned buf[4][ZS_ROW_DW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* w = buf[wave];
  unsigned over = 0;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    const zs_u2 x = __builtin_nontemporal_load(reinterpret_cast<const zs_u2*>(in + r * 128) + lane);
    const bool b0 = x[0] != 0u, b1 = x[1] != 0u;
    const unsigned long long m0 = __ballot(b0), m1 = __ballot(b1);
    const int n0 = __builtin_popcountll(m0), n1 = __builtin_popcountll(m1);
    const bool fits = n0 <= ZS_CAP && n1 <= ZS_CAP;  // wave-uniform
    if (lane < ZS_ROW_DW / 2) {
      zs_u2 z = {0u, 0u};
      if (lane == 0) z = zs_u2{(unsigned)m0, (unsigned)(m0 >> 32)};
      if (lane == 1) z = zs_u2{(unsigned)m1, (unsigned)(m1 >> 32)};
      *reinterpret_cast<zs_u2*>(w + 2 * lane) = z;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (fits) {
      const unsigned k0 = __builtin_amdgcn_mbcnt_hi((unsigned)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m0, 0u));
      const unsigned k1 = __builtin_amdgcn_mbcnt_hi((unsigned)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m1, 0u));
      if (b0) w[4 + 2 * k0] = x[0];
      if (b1) w[5 + 2 * k1] = x[1];
    } else {
      ++over;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane < ZS_ROW_DW / 2) {
      const zs_u2 o = *reinterpret_cast<const zs_u2*>(w + 2 * lane);
      __builtin_nontemporal_store(o, reinterpret_cast<zs_u2*>(out + r * ZS_ROW_DW) + lane);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  if (overflow && over > 0 && lane == 0) atomicAdd(overflow, over);  // (a vector atomic, once per wave)
}

// (tests and tools: not on any hot path)
__global__ __launch_bounds__(256) void unpack_zs_kernel(int64_t rows, const unsigned* __restrict__ zs, const float* __restrict__ dense,
                                                         float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) unsigned buf[4][ZS_ROW_DW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* w = buf[wave];
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    if (lane < ZS_ROW_DW / 2) *reinterpret_cast<zs_u2*>(w + 2 * lane) = reinterpret_cast<const zs_u2*>(zs + r * ZS_ROW_DW)[lane];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const unsigned long long m0 = ((unsigned long long)w[1] << 32) | w[0], m1 = ((unsigned long long)w[3] << 32) | w[2];
    const int n0 = __builtin_popcountll(m0), n1 = __builtin_popcountll(m1);
    zs_u2 v;
    if (n0 > ZS_CAP || n1 > ZS_CAP) {
      v = reinterpret_cast<const zs_u2*>(dense + r * 128)[lane];
    } else {
      const unsigned p0 = 4u + 2u * (unsigned)__builtin_popcountll(m0 & ((1ull << lane) - 1ull));
      const unsigned p1 = 5u + 2u * (unsigned)__builtin_popcountll(m1 & ((1ull << lane) - 1ull));
      v[0] = ((m0 >> lane) & 1ull) ? w[p0 < (unsigned)ZS_ROW_DW ? p0 : 0u] : 0u;
      v[1] = ((m1 >> lane) & 1ull) ? w[p1 < (unsigned)ZS_ROW_DW ? p1 : 0u] : 0u;
    }
    reinterpret_cast<zs_u2*>(out + r * 128)[lane] = v;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// ---- wide zero-suppressed tables: rows of 256 floats, one image per 128-column K-slab ------------------------------------
// The aggregation of a 256-column table runs as two 128-column K-slab launches (spmm.hip), so the table packs as two independent
// images, slab-major: [2][rows][384 B], image s bit for bit what pack_zs_kernel writes for columns 128 s .. 128 s + 127.  One pass
// over the table, one wave per row: two 8-B loads per lane (one per slab), each slab's row put together in its own 384 B of the
// wave's LDS and stored as three whole lines.  `overflow` counts over-capacity ROW-SLABS (a row can count twice).
__global__ __launch_bounds__(256) void pack_zs_wide_kernel(int64_t rows, const float* __restrict__ in, unsigned* __restrict__ out,
                                                            unsigned* __restrict__ overflow) {
  __shared__ __attribute__((aligned(16))) unsigned buf[4][2][ZS_ROW_DW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned over = 0;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    zs_u2 x[2];
    bool b0[2], b1[2], fits[2];
    unsigned long long m0[2], m1[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) x[s] = __builtin_nontemporal_load(reinterpret_cast<const zs_u2*>(in + r * 256 + 128 * s) + lane);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      unsigned* w = buf[wave][s];
      b0[s] = x[s][0] != 0u;
      b1[s] = x[s][1] != 0u;
      m0[s] = __ballot(b0[s]);
      m1[s] = __ballot(b1[s]);
      fits[s] = __builtin_popcountll(m0[s]) <= ZS_CAP && __builtin_popcountll(m1[s]) <= ZS_CAP;  // wave-uniform
      if (lane < ZS_ROW_DW / 2) {
        zs_u2 z = {0u, 0u};
        if (lane == 0) z = zs_u2{(unsigned)m0[s], (unsigned)(m0[s] >> 32)};
        if (lane == 1) z = zs_u2{(unsigned)m1[s], (unsigned)(m1[s] >> 32)};
        *reinterpret_cast<zs_u2*>(w + 2 * lane) = z;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      unsigned* w = buf[wave][s];
      if (fits[s]) {
        const unsigned k0 = __builtin_amdgcn_mbcnt_hi((unsigned)(m0[s] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m0[s], 0u));
        const unsigned k1 = __builtin_amdgcn_mbcnt_hi((unsigned)(m1[s] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m1[s], 0u));
        if (b0[s]) w[4 + 2 * k0] = x[s][0];
        if (b1[s]) w[5 + 2 * k1] = x[s][1];
      } else {
        ++over;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane < ZS_ROW_DW / 2) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const zs_u2 o = *reinterpret_cast<const zs_u2*>(buf[wave][s] + 2 * lane);
        __builtin_nontemporal_store(o, reinterpret_cast<zs_u2*>(out + ((int64_t)s * rows + r) * ZS_ROW_DW) + lane);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  if (overflow && over > 0 && lane == 0) atomicAdd(overflow, over);  // (a vector atomic, once per wave)
}

// (tests and tools: not on any hot path) blockIdx.y = slab
__global__ __launch_bounds__(256) void unpack_zs_wide_kernel(int64_t rows, const unsigned* __restrict__ zs, const float* __restrict__ dense,
                                                              float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) unsigned buf[4][ZS_ROW_DW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.y;
  unsigned* w = buf[wave];
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
    if (lane < ZS_ROW_DW / 2)
      *reinterpret_cast<zs_u2*>(w + 2 * lane) = reinterpret_cast<const zs_u2*>(zs + ((int64_t)s * rows + r) * ZS_ROW_DW)[lane];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const unsigned long long m0 = ((unsigned long long)w[1] << 32) | w[0], m1 = ((unsigned long long)w[3] << 32) | w[2];
    const int n0 = __builtin_popcountll(m0), n1 = __builtin_popcountll(m1);
    zs_u2 v;
    if (n0 > ZS_CAP || n1 > ZS_CAP) {
      v = reinterpret_cast<const zs_u2*>(dense + r * 256 + 128 * s)[lane];
    } else {
      const unsigned p0 = 4u + 2u * (unsigned)__builtin_popcountll(m0 & ((1ull << lane) - 1ull));
      const unsigned p1 = 5u + 2u * (unsigned)__builtin_popcountll(m1 & ((1ull << lane) - 1ull));
      v[0] = ((m0 >> lane) & 1ull) ? w[p0 < (unsigned)ZS_ROW_DW ? p0 : 0u] : 0u;
      v[1] = ((m1 >> lane) & 1ull) ? w[p1 < (unsigned)ZS_ROW_DW ? p1 : 0u] : 0u;
    }
    reinterpret_cast<zs_u2*>(out + r * 256 + 128 * s)[lane] = v;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// ---- fp8 tables with per-row scales (include/gaib.h) ----------------------------------------------------------
// Row r becomes ld bytes of OCP e4m3 "fn" and scale[r] = 2^k: k the smallest integer with amax * 2^-k <= 448 (amax over the
// row's finite elements), clamped to [-126, 120], 0 for a row without a non-zero finite element.  On the bits of amax = 1.m x
// 2^(e - 127): 448 = 1.75 x 2^8, so k = e - 127 - 8, one more where 1.m > 1.75; a subnormal amax is far below the lower clamp.
__device__ __forceinline__ int fp8_row_exponent(unsigned amax_bits) {
  if (amax_bits == 0u) return 0;
  const int e = (int)(amax_bits >> 23);
  if (e == 0) return -126;
  const int k = e - 135 + ((amax_bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  return k < -126 ? -126 : (k > 120 ? 120 : k);
}
// four elements times 2^-k (exact) as four e4m3 bytes, round to nearest even (v_cvt_pk_fp8_f32); magnitudes above 448 saturate,
// a NaN or an infinity becomes the NaN of its sign (0x7f / 0xff: the format has no infinity); columns >= nvalid are pad: byte 0
__device__ __forceinline__ unsigned fp8_quant4(const float (&v)[4], float inv, int nvalid) {
  float s[4];
  unsigned fix_mask = 0u, fix_val = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    s[k] = v[k] * inv;
    const unsigned b = __float_as_uint(s[k]);
    if ((b & 0x7fffffffu) >= 0x7f800000u) {
      fix_mask |= 0xffu << (8 * k);
      fix_val |= (0x7fu | ((b >> 24) & 0x80u)) << (8 * k);
      s[k] = 0.f;
    } else {
      s[k] = fminf(fmaxf(s[k], -448.f), 448.f);
    }
    if (k >= nvalid) {
      fix_mask |= 0xffu << (8 * k);
      fix_val &= ~(0xffu << (8 * k));
      s[k] = 0.f;
    }
  }
  int p = 0;
  p = __builtin_amdgcn_cvt_pk_fp8_f32(s[0], s[1], p, false);
  p = __builtin_amdgcn_cvt_pk_fp8_f32(s[2], s[3], p, true);
  return ((unsigned)p & ~fix_mask) | fix_val;
}
// One wave per row, a lane per 4 consecutive columns (one 4-B store; ld % 4 == 0): the row's amax by a wave reduction, then the
// conversion.  The lane's first four values stay in registers between the two passes (rows up to 256 columns are read once);
// wider rows read the rest again, from the cache.  VIN: 16-B loads (in 16-B aligned, len % 4 == 0).
template <bool VIN>
__global__ __launch_bounds__(256) void cast_f32_fp8_rows_kernel(int64_t rows, int len, int64_t ld, const float* __restrict__ in,
                                                                uint8_t* __restrict__ q, float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int ngroups = (int)(ld / 4);
  auto load4 = [&](const float* src, int c, float (&v)[4]) {
    if (VIN && c + 4 <= len) {
      const f4 a = *reinterpret_cast<const f4*>(src + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = a[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = c + k < len ? src[c + k] : 0.f;
    }
  };
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    const float* src = in + r * len;
    float v0[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned amax = 0u;
    for (int gq = lane; gq < ngroups; gq += 64) {
      float v[4];
      load4(src, 4 * gq, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (gq == lane) v0[k] = v[k];
        const unsigned b = __float_as_uint(v[k]) & 0x7fffffffu;
        if (b < 0x7f800000u) amax = b > amax ? b : amax;  // (the bit patterns of non-negative floats order as the values do)
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned t = (unsigned)__shfl_xor((int)amax, o, 64);
      amax = t > amax ? t : amax;
    }
    const int k2 = fp8_row_exponent(amax);
    const float inv = __uint_as_float((unsigned)(127 - k2) << 23);
    if (lane == 0) scale[r] = __uint_as_float((unsigned)(127 + k2) << 23);
    unsigned* dst = reinterpret_cast<unsigned*>(q + r * ld);
    for (int gq = lane; gq < ngroups; gq += 64) {
      float v[4];
      if (gq == lane) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v0[k];
      } else {
        load4(src, 4 * gq, v);
      }
      dst[gq] = fp8_quant4(v, inv, len - 4 * gq);
    }
  }
}
// the exact widening into dense rows: out[r][c] = f32(q[r][c]) * scale[r]
__global__ __launch_bounds__(256) void cast_fp8_f32_rows_kernel(int64_t n, int len, int64_t ld, const uint8_t* __restrict__ q,
                                                                const float* __restrict__ scale, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t r = i / len;
    const int64_t c = i - r * len;
    const unsigned b = q[r * ld + c];
    // (a NaN byte becomes the quiet NaN of ITS sign: the conversion instruction and the product both hand back one default NaN)
    out[i] = (b & 0x7fu) == 0x7fu ? __uint_as_float(0x7fc00000u | ((b << 24) & 0x80000000u)) : __builtin_amdgcn_cvt_f32_fp8((int)b, 0) * scale[r];
  }
}

}  // namespace

extern "C" int gaib_fill_f32(gaib_ctx* ctx, int64_t n, float value, float* d_x) {
  GAIB_CHECK(ctx && (d_x || n == 0), "gaib_fill_f32: NULL argument");
  if (n <= 0) return GAIB_OK;
  fill_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, value, d_x);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_scale_f32(gaib_ctx* ctx, int64_t n, float alpha, float* d_x) {
  GAIB_CHECK(ctx && (d_x || n == 0), "gaib_scale_f32: NULL argument");
  if (n <= 0) return GAIB_OK;
  scale_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, alpha, d_x);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_cast_f32_bf16(gaib_ctx* ctx, int64_t n, const float* d_in, uint16_t* d_out) {
  GAIB_CHECK(ctx && ((d_in && d_out) || n == 0), "gaib_cast_f32_bf16: NULL argument");
  GAIB_CHECK(n >= 0, "gaib_cast_f32_bf16: n < 0");
  if (n == 0) return GAIB_OK;
  GAIB_CHECK((const void*)d_in != (const void*)d_out, "gaib_cast_f32_bf16: in and out must not alias");
  const int vec = ((((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0);
  ProfScope ps(ctx, "cast_f32_bf16", 6.0 * (double)n);
  if (vec) cast_f32_bf16_kernel<<<stream_grid(n / 8 + 1, 256), 256, 0, ctx->stream>>>(n, d_in, d_out, 1);
  else cast_f32_bf16_scalar_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, d_in, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_cast_f32_bf16_rows(gaib_ctx* ctx, int64_t rows, int len, const float* d_in, int64_t ld_out, uint16_t* d_out) {
  GAIB_CHECK(ctx, "gaib_cast_f32_bf16_rows: NULL ctx");
  GAIB_CHECK(rows >= 0 && len >= 0, "gaib_cast_f32_bf16_rows: rows or len < 0");
  GAIB_CHECK(ld_out >= len, "gaib_cast_f32_bf16_rows: ld_out (%lld) below len (%d)", (long long)ld_out, len);
  if (rows == 0 || ld_out == 0) return GAIB_OK;
  if (ld_out == len) return gaib_cast_f32_bf16(ctx, rows * len, d_in, d_out);  // dense rows: the flat cast
  GAIB_CHECK(d_out && (d_in || len == 0), "gaib_cast_f32_bf16_rows: NULL argument");
  GAIB_CHECK((const void*)d_in != (const void*)d_out, "gaib_cast_f32_bf16_rows: in and out must not alias");
  const int64_t n = rows * ld_out;
  ProfScope ps(ctx, "cast_f32_bf16", 4.0 * (double)rows * len + 2.0 * (double)n);
  if (ld_out % 8 == 0 && ((uintptr_t)d_out & 15) == 0 && ld_out / 8 <= 0x7fffffff) {
    const bool vin = len % 4 == 0 && ((uintptr_t)d_in & 15) == 0;
    const unsigned grid = stream_grid(n / 8, 256);
    if (vin) cast_f32_bf16_rows_kernel<true><<<grid, 256, 0, ctx->stream>>>(n / 8, len, (int)(ld_out / 8), d_in, d_out);
    else cast_f32_bf16_rows_kernel<false><<<grid, 256, 0, ctx->stream>>>(n / 8, len, (int)(ld_out / 8), d_in, d_out);
  } else {
    cast_f32_bf16_rows_scalar_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, len, ld_out, d_in, d_out);
  }
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_cast_bf16_f32(gaib_ctx* ctx, int64_t n, const uint16_t* d_in, float* d_out) {
  GAIB_CHECK(ctx && ((d_in && d_out) || n == 0), "gaib_cast_bf16_f32: NULL argument");
  GAIB_CHECK(n >= 0, "gaib_cast_bf16_f32: n < 0");
  if (n == 0) return GAIB_OK;
  GAIB_CHECK((const void*)d_in != (const void*)d_out, "gaib_cast_bf16_f32: in and out must not alias");
  const int vec = ((((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0);
  ProfScope ps(ctx, "cast_bf16_f32", 6.0 * (double)n);
  if (vec) cast_bf16_f32_kernel<<<stream_grid(n / 8 + 1, 256), 256, 0, ctx->stream>>>(n, d_in, d_out, 1);
  else cast_bf16_f32_scalar_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, d_in, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// No host wait and no allocation in either fp8 cast: both are legal inside a stream capture.
extern "C" int gaib_cast_f32_fp8_rows(gaib_ctx* ctx, int64_t rows, int len, const float* d_in, int64_t ld, uint8_t* d_q, float* d_scale) {
  GAIB_CHECK(ctx, "gaib_cast_f32_fp8_rows: NULL ctx");
  GAIB_CHECK(rows >= 0 && len >= 0, "gaib_cast_f32_fp8_rows: rows or len < 0");
  GAIB_CHECK(ld >= len && ld % 4 == 0, "gaib_cast_f32_fp8_rows: row stride ld (%lld bytes) must be a multiple of 4 not below len (%d)",
             (long long)ld, len);
  if (rows == 0) return GAIB_OK;
  GAIB_CHECK(d_scale && (d_q || ld == 0) && (d_in || len == 0), "gaib_cast_f32_fp8_rows: NULL argument");
  GAIB_CHECK(((uintptr_t)d_q & 3) == 0, "gaib_cast_f32_fp8_rows: the fp8 table must be 4-byte aligned (16 for the aggregation calls)");
  GAIB_CHECK((const void*)d_in != (const void*)d_q && (const void*)d_in != (const void*)d_scale, "gaib_cast_f32_fp8_rows: in and out must not alias");
  ProfScope ps(ctx, "cast_f32_fp8", (double)rows * (4.0 * len + (double)ld + 4.0));
  const unsigned grid = (unsigned)std::min<int64_t>((rows + 3) / 4, (int64_t)ctx->num_cus * 64);
  if (len % 4 == 0 && ((uintptr_t)d_in & 15) == 0) cast_f32_fp8_rows_kernel<true><<<grid, 256, 0, ctx->stream>>>(rows, len, ld, d_in, d_q, d_scale);
  else cast_f32_fp8_rows_kernel<false><<<grid, 256, 0, ctx->stream>>>(rows, len, ld, d_in, d_q, d_scale);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_cast_fp8_f32_rows(gaib_ctx* ctx, int64_t rows, int len, int64_t ld, const uint8_t* d_q, const float* d_scale,
                                      float* d_out) {
  GAIB_CHECK(ctx, "gaib_cast_fp8_f32_rows: NULL ctx");
  GAIB_CHECK(rows >= 0 && len >= 0 && ld >= len, "gaib_cast_fp8_f32_rows: rows or len < 0, or ld below len");
  if (rows == 0 || len == 0) return GAIB_OK;
  GAIB_CHECK(d_q && d_scale && d_out, "gaib_cast_fp8_f32_rows: NULL argument");
  GAIB_CHECK((const void*)d_q != (const void*)d_out && (const void*)d_scale != (const void*)d_out, "gaib_cast_fp8_f32_rows: in and out must not alias");
  const int64_t n = rows * len;
  ProfScope ps(ctx, "cast_fp8_f32", 5.0 * (double)n + 4.0 * (double)rows);
  cast_fp8_f32_rows_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, len, ld, d_q, d_scale, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_pack_zs(gaib_ctx* ctx, int64_t rows, int len, const float* d_in, void* d_zs, uint32_t* d_overflow) {
  GAIB_CHECK(ctx && ((d_in && d_zs) || rows == 0), "gaib_pack_zs: NULL argument");
  GAIB_CHECK(rows >= 0, "gaib_pack_zs: rows < 0");
  if (len != 128) {
    gaib_set_error("gaib_pack_zs: rows of %d columns (the zero-suppressed format holds rows of 128)", len);
    return GAIB_ERR_UNSUPPORTED;
  }
  if (rows == 0) return GAIB_OK;
  GAIB_CHECK(((uintptr_t)d_in & 7) == 0 && ((uintptr_t)d_zs & 127) == 0, "gaib_pack_zs: the table must sit on an 8-B, the image on a 128-B boundary");
  GAIB_CHECK((const void*)d_in != (const void*)d_zs, "gaib_pack_zs: in and out must not alias");
  ProfScope ps(ctx, "pack_zs", (512.0 + 384.0) * (double)rows);
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(rows, 4), (int64_t)ctx->num_cus * 32);
  pack_zs_kernel<<<grid, 256, 0, ctx->stream>>>(rows, d_in, static_cast<unsigned*>(d_zs), d_overflow);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_unpack_zs(gaib_ctx* ctx, int64_t rows, int len, const void* d_zs, const float* d_dense, float* d_out) {
  GAIB_CHECK(ctx && ((d_zs && d_dense && d_out) || rows == 0), "gaib_unpack_zs: NULL argument");
  GAIB_CHECK(rows >= 0, "gaib_unpack_zs: rows < 0");
  if (len != 128) {
    gaib_set_error("gaib_unpack_zs: rows of %d columns (the zero-suppressed format holds rows of 128)", len);
    return GAIB_ERR_UNSUPPORTED;
  }
  if (rows == 0) return GAIB_OK;
  GAIB_CHECK((((uintptr_t)d_dense | (uintptr_t)d_out | (uintptr_t)d_zs) & 7) == 0, "gaib_unpack_zs: tables must sit on 8-B boundaries");
  GAIB_CHECK(d_dense != d_out, "gaib_unpack_zs: dense and out must not alias");
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(rows, 4), (int64_t)ctx->num_cus * 32);
  unpack_zs_kernel<<<grid, 256, 0, ctx->stream>>>(rows, static_cast<const unsigned*>(d_zs), d_dense, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_pack_zs_wide(gaib_ctx* ctx, int64_t rows, int len, const float* d_in, void* d_zs, uint32_t* d_overflow) {
  GAIB_CHECK(ctx && ((d_in && d_zs) || rows == 0), "gaib_pack_zs_wide: NULL argument");
  GAIB_CHECK(rows >= 0, "gaib_pack_zs_wide: rows < 0");
  if (len != 256) {
    gaib_set_error("gaib_pack_zs_wide: rows of %d columns (the wide zero-suppressed format holds rows of 256: two slabs of 128)", len);
    return GAIB_ERR_UNSUPPORTED;
  }
  if (rows == 0) return GAIB_OK;
  GAIB_CHECK(((uintptr_t)d_in & 7) == 0 && ((uintptr_t)d_zs & 127) == 0, "gaib_pack_zs_wide: the table must sit on an 8-B, the image on a 128-B boundary");
  GAIB_CHECK((const void*)d_in != (const void*)d_zs, "gaib_pack_zs_wide: in and out must not alias");
  ProfScope ps(ctx, "pack_zs_wide", (1024.0 + 768.0) * (double)rows);
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(rows, 4), (int64_t)ctx->num_cus * 32);
  pack_zs_wide_kernel<<<grid, 256, 0, ctx->stream>>>(rows, d_in, static_cast<unsigned*>(d_zs), d_overflow);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_unpack_zs_wide(gaib_ctx* ctx, int64_t rows, int len, const void* d_zs, const float* d_dense, float* d_out) {
  GAIB_CHECK(ctx && ((d_zs && d_dense && d_out) || rows == 0), "gaib_unpack_zs_wide: NULL argument");
  GAIB_CHECK(rows >= 0, "gaib_unpack_zs_wide: rows < 0");
  if (len != 256) {
    gaib_set_error("gaib_unpack_zs_wide: rows of %d columns (the wide zero-suppressed format holds rows of 256: two slabs of 128)", len);
    return GAIB_ERR_UNSUPPORTED;
  }
  if (rows == 0) return GAIB_OK;
  GAIB_CHECK((((uintptr_t)d_dense | (uintptr_t)d_out | (uintptr_t)d_zs) & 7) == 0, "gaib_unpack_zs_wide: tables must sit on 8-B boundaries");
  GAIB_CHECK(d_dense != d_out, "gaib_unpack_zs_wide: dense and out must not alias");
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(rows, 4), (int64_t)ctx->num_cus * 32);
  unpack_zs_wide_kernel<<<dim3(grid, 2), 256, 0, ctx->stream>>>(rows, static_cast<const unsigned*>(d_zs), d_dense, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_relu(gaib_ctx* ctx, int64_t n, const float* d_in, float* d_out) {
  GAIB_CHECK(ctx && ((d_in && d_out) || n == 0), "gaib_relu: NULL argument");
  if (n <= 0) return GAIB_OK;
  const int vec_ok = ((((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0);
  ProfScope ps(ctx, "relu", 8.0 * (double)n);
  relu_kernel<<<stream_grid(n / 4 + 1, 256), 256, 0, ctx->stream>>>(n, d_in, d_out, vec_ok);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_d_relu(gaib_ctx* ctx, int64_t n, const float* d_in_diff, const float* d_data,
                           float* d_out_diff) {
  GAIB_CHECK(ctx && ((d_in_diff && d_data && d_out_diff) || n == 0), "gaib_d_relu: NULL argument");
  if (n <= 0) return GAIB_OK;
  const int vec_ok = ((((uintptr_t)d_in_diff | (uintptr_t)d_data | (uintptr_t)d_out_diff) & 15) == 0);
  ProfScope ps(ctx, "d_relu", 12.0 * (double)n);
  d_relu_kernel<<<stream_grid(n / 4 + 1, 256), 256, 0, ctx->stream>>>(n, d_in_diff, d_data,
                                                                     d_out_diff, vec_ok);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_dropout(gaib_ctx* ctx, int64_t n, float scale, float drop_rate, uint64_t seed,
                            const float* d_in, uint8_t* d_masks, float* d_out) {
  GAIB_CHECK(ctx && ((d_in && d_masks && d_out) || n == 0), "gaib_dropout: NULL argument");
  GAIB_CHECK(drop_rate >= 0.f && drop_rate < 1.f, "gaib_dropout: rate must be in [0,1)");
  if (n <= 0) return GAIB_OK;
  dropout_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, scale, drop_rate, seed, d_in,
                                                               d_masks, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_dropout_dev(gaib_ctx* ctx, int64_t n, float scale, float drop_rate, uint64_t* d_seed,
                                const float* d_in, uint8_t* d_masks, float* d_out) {
  GAIB_CHECK(ctx && d_seed && ((d_in && d_masks && d_out) || n == 0), "gaib_dropout_dev: NULL argument");
  GAIB_CHECK(drop_rate >= 0.f && drop_rate < 1.f, "gaib_dropout_dev: rate must be in [0,1)");
  GAIB_CHECK(((uintptr_t)d_seed & 7) == 0, "gaib_dropout_dev: d_seed must be 8-byte aligned");
  if (n > 0) {
    const int vec_ok = ((((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0) && (((uintptr_t)d_masks & 3) == 0);
    dropout_dev_kernel<<<stream_grid(n / 4 + 1, 256), 256, 0, ctx->stream>>>(n, scale, drop_rate, d_seed, d_in, d_masks,
                                                                            d_out, vec_ok);
    GAIB_LAUNCH_CHECK();
  }
  seed_advance_kernel<<<1, 1, 0, ctx->stream>>>(d_seed);  // once per call, also for n == 0 (the host's seed++ runs whatever n is)
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_d_dropout(gaib_ctx* ctx, int64_t n, float scale, const float* d_in,
                              const uint8_t* d_masks, float* d_out) {
  GAIB_CHECK(ctx && ((d_in && d_masks && d_out) || n == 0), "gaib_d_dropout: NULL argument");
  if (n <= 0) return GAIB_OK;
  d_dropout_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, scale, d_in, d_masks, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_softmax_xent(gaib_ctx* ctx, int num_cls, int64_t begin, int64_t end,
                                 const float* d_in, const uint8_t* d_masks, const uint8_t* d_labels,
                                 float* d_loss, float* d_out) {
  GAIB_CHECK(ctx && d_in && d_labels && d_loss && d_out, "gaib_softmax_xent: NULL argument");
  GAIB_CHECK(num_cls > 0 && begin >= 0 && end >= begin, "gaib_softmax_xent: bad range");
  if (end == begin) return GAIB_OK;
  softmax_xent_kernel<<<(unsigned)cdiv64(end - begin, 4), 256, 0, ctx->stream>>>(
      num_cls, begin, end, d_in, d_masks, d_labels, d_loss, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_d_softmax_xent(gaib_ctx* ctx, int num_cls, int64_t begin, int64_t end,
                                   const uint8_t* d_masks, const uint8_t* d_labels,
                                   const float* d_out, float* d_diff) {
  GAIB_CHECK(ctx && d_labels && d_out && d_diff, "gaib_d_softmax_xent: NULL argument");
  GAIB_CHECK(num_cls > 0 && begin >= 0 && end >= begin, "gaib_d_softmax_xent: bad range");
  if (end == begin) return GAIB_OK;
  d_softmax_xent_kernel<<<stream_grid((end - begin) * num_cls, 256), 256, 0, ctx->stream>>>(
      num_cls, begin, end, d_masks, d_labels, d_out, d_diff);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_sigmoid_xent(gaib_ctx* ctx, int num_cls, int64_t begin, int64_t end,
                                 const float* d_in, const uint8_t* d_masks, const uint8_t* d_labels,
                                 float* d_loss, float* d_out) {
  GAIB_CHECK(ctx && d_in && d_labels && d_loss && d_out, "gaib_sigmoid_xent: NULL argument");
  GAIB_CHECK(num_cls > 0 && begin >= 0 && end >= begin, "gaib_sigmoid_xent: bad range");
  if (end == begin) return GAIB_OK;
  sigmoid_xent_kernel<<<(unsigned)cdiv64(end - begin, 4), 256, 0, ctx->stream>>>(
      num_cls, begin, end, d_in, d_masks, d_labels, d_loss, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_d_sigmoid_xent(gaib_ctx* ctx, int num_cls, int64_t begin, int64_t end,
                                   const uint8_t* d_masks, const uint8_t* d_labels,
                                   const float* d_out, float* d_diff) {
  GAIB_CHECK(ctx && d_labels && d_out && d_diff, "gaib_d_sigmoid_xent: NULL argument");
  GAIB_CHECK(num_cls > 0 && begin >= 0 && end >= begin, "gaib_d_sigmoid_xent: bad range");
  if (end == begin) return GAIB_OK;
  d_sigmoid_xent_kernel<<<stream_grid((end - begin) * num_cls, 256), 256, 0, ctx->stream>>>(
      num_cls, begin, end, d_masks, d_labels, d_out, d_diff);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_masked_f1_micro(gaib_ctx* ctx, int64_t begin, int64_t end, int num_cls,
                                    const uint8_t* d_masks, const float* d_preds,
                                    const uint8_t* d_labels, float* h_result, int64_t* h_counts) {
  GAIB_CHECK(ctx && d_preds && d_labels && h_result, "gaib_masked_f1_micro: NULL argument");
  GAIB_CHECK(begin >= 0 && end >= begin && num_cls > 0, "gaib_masked_f1_micro: bad range");
  GAIB_NOT_WHILE_CAPTURING(ctx, "gaib_masked_f1_micro (use gaib_masked_f1_counts_dev)");
  *h_result = 0.f;
  unsigned long long c[3] = {0, 0, 0};
  if (end > begin) {
    GAIB_TRY(gaib_ws_reserve(ctx, sizeof(c)));
    GAIB_HIP(hipMemsetAsync(ctx->ws, 0, sizeof(c), ctx->stream));
    unsigned grid = stream_grid((end - begin) * num_cls, 256);
    f1_counts_kernel<<<grid, 256, 0, ctx->stream>>>(num_cls, begin, end, d_masks, d_preds, d_labels,
                                                    (unsigned long long*)ctx->ws);
    GAIB_LAUNCH_CHECK();
    GAIB_HIP(hipMemcpyAsync(c, ctx->ws, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    GAIB_HIP(hipStreamSynchronize(ctx->stream));
  }
  const double tp = (double)c[0], fp = (double)c[1], fn = (double)c[2];
  const double prec = tp + fp > 0 ? tp / (tp + fp) : 0.;
  const double rec = tp + fn > 0 ? tp / (tp + fn) : 0.;
  *h_result = (float)(rec + prec > 0. ? 2. * (rec * prec) / (rec + prec) : 0.);
  if (h_counts) {
    h_counts[0] = (int64_t)c[0];
    h_counts[1] = (int64_t)c[1];
    h_counts[2] = (int64_t)c[2];
  }
  return GAIB_OK;
}

extern "C" int gaib_masked_avg_loss(gaib_ctx* ctx, int64_t begin, int64_t end,
                                    const uint8_t* d_masks, const float* d_loss, float* h_result) {
  GAIB_CHECK(ctx && d_loss && h_result, "gaib_masked_avg_loss: NULL argument");
  GAIB_CHECK(begin >= 0 && end >= begin, "gaib_masked_avg_loss: bad range");
  *h_result = 0.f;
  if (end == begin) return GAIB_OK;
  const int nblocks = (int)stream_grid(end - begin, 256) > 1024 ? 1024 : (int)stream_grid(end - begin, 256);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * 2 * 1024));
  masked_loss_partial_kernel<<<nblocks, 256, 0, ctx->stream>>>(begin, end, d_masks, d_loss,
                                                               (float*)ctx->ws);
  GAIB_LAUNCH_CHECK();
  return finish_partial(ctx, nblocks, (float*)ctx->ws, h_result);
}

extern "C" int gaib_masked_accuracy_single(gaib_ctx* ctx, int64_t begin, int64_t end, int num_cls,
                                           const uint8_t* d_masks, const float* d_preds,
                                           const uint8_t* d_labels, float* h_result) {
  GAIB_CHECK(ctx && d_preds && d_labels && h_result, "gaib_masked_accuracy_single: NULL argument");
  GAIB_CHECK(begin >= 0 && end >= begin && num_cls > 0, "gaib_masked_accuracy_single: bad range");
  *h_result = 0.f;
  if (end == begin) return GAIB_OK;
  const int nblocks = (int)stream_grid(end - begin, 256) > 1024 ? 1024 : (int)stream_grid(end - begin, 256);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * 2 * 1024));
  masked_acc_partial_kernel<<<nblocks, 256, 0, ctx->stream>>>(begin, end, num_cls, d_masks, d_preds,
                                                              d_labels, (float*)ctx->ws);
  GAIB_LAUNCH_CHECK();
  return finish_partial(ctx, nblocks, (float*)ctx->ws, h_result);
}

// tp, fp, fn of the multi-label head left in device memory (d_counts[3], 64-bit); the F1 is the caller's arithmetic
extern "C" int gaib_masked_f1_counts_dev(gaib_ctx* ctx, int64_t begin, int64_t end, int num_cls, const uint8_t* d_masks,
                                         const float* d_preds, const uint8_t* d_labels, uint64_t* d_counts) {
  GAIB_CHECK(ctx && d_preds && d_labels && d_counts, "gaib_masked_f1_counts_dev: NULL argument");
  GAIB_CHECK(begin >= 0 && end >= begin && num_cls > 0, "gaib_masked_f1_counts_dev: bad range");
  GAIB_HIP(hipMemsetAsync(d_counts, 0, 3 * sizeof(uint64_t), ctx->stream));
  if (end > begin) {
    unsigned grid = stream_grid((end - begin) * num_cls, 256);
    f1_counts_kernel<<<grid, 256, 0, ctx->stream>>>(num_cls, begin, end, d_masks, d_preds, d_labels,
                                                    (unsigned long long*)d_counts);
    GAIB_LAUNCH_CHECK();
  }
  return GAIB_OK;
}

// the two metrics with the result left in DEVICE memory (d_result[0]); no host wait, recordable
extern "C" int gaib_masked_avg_loss_dev(gaib_ctx* ctx, int64_t begin, int64_t end, const uint8_t* d_masks,
                                        const float* d_loss, float* d_result) {
  GAIB_CHECK(ctx && d_loss && d_result, "gaib_masked_avg_loss_dev: NULL argument");
  GAIB_CHECK(begin >= 0 && end >= begin, "gaib_masked_avg_loss_dev: bad range");
  if (end == begin) return gaib_fill_f32(ctx, 1, 0.f, d_result);
  const int nblocks = (int)stream_grid(end - begin, 256) > 1024 ? 1024 : (int)stream_grid(end - begin, 256);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * 2 * 1024));
  masked_loss_partial_kernel<<<nblocks, 256, 0, ctx->stream>>>(begin, end, d_masks, d_loss, (float*)ctx->ws);
  GAIB_LAUNCH_CHECK();
  finish_partial_kernel<<<1, 256, 0, ctx->stream>>>(nblocks, (const float*)ctx->ws, d_result);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_masked_accuracy_single_dev(gaib_ctx* ctx, int64_t begin, int64_t end, int num_cls,
                                               const uint8_t* d_masks, const float* d_preds,
                                               const uint8_t* d_labels, float* d_result) {
  GAIB_CHECK(ctx && d_preds && d_labels && d_result, "gaib_masked_accuracy_single_dev: NULL argument");
  GAIB_CHECK(begin >= 0 && end >= begin && num_cls > 0, "gaib_masked_accuracy_single_dev: bad range");
  if (end == begin) return gaib_fill_f32(ctx, 1, 0.f, d_result);
  const int nblocks = (int)stream_grid(end - begin, 256) > 1024 ? 1024 : (int)stream_grid(end - begin, 256);
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * 2 * 1024));
  masked_acc_partial_kernel<<<nblocks, 256, 0, ctx->stream>>>(begin, end, num_cls, d_masks, d_preds, d_labels,
                                                              (float*)ctx->ws);
  GAIB_LAUNCH_CHECK();
  finish_partial_kernel<<<1, 256, 0, ctx->stream>>>(nblocks, (const float*)ctx->ws, d_result);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_l2norm(gaib_ctx* ctx, int64_t n, int dim, const float* d_in, float* d_out) {
  GAIB_CHECK(ctx && ((d_in && d_out) || n == 0), "gaib_l2norm: NULL argument");
  if (n <= 0 || dim <= 0) return GAIB_OK;
  l2norm_kernel<<<(unsigned)cdiv64(n, 4), 256, 0, ctx->stream>>>(n, dim, d_in, d_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_d_l2norm(gaib_ctx* ctx, int64_t n, int dim, const float* d_feat_in,
                             const float* d_grad_in, float* d_grad_out) {
  GAIB_CHECK(ctx && ((d_feat_in && d_grad_in && d_grad_out) || n == 0), "gaib_d_l2norm: NULL argument");
  if (n <= 0 || dim <= 0) return GAIB_OK;
  d_l2norm_kernel<<<(unsigned)cdiv64(n, 4), 256, 0, ctx->stream>>>(n, dim, d_feat_in, d_grad_in,
                                                                   d_grad_out);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_adam_step(gaib_ctx* ctx, int64_t n, const float* d_dW, float* d_W, float* d_m,
                              float* d_v, float alpha, float b1, float b2, float b1_t, float b2_t,
                              float eps) {
  GAIB_CHECK(ctx && ((d_dW && d_W && d_m && d_v) || n == 0), "gaib_adam_step: NULL argument");
  if (n <= 0) return GAIB_OK;
  adam_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, d_dW, d_W, d_m, d_v, alpha, b1, b2,
                                                            b1_t, b2_t, eps);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_adam_step_dev(gaib_ctx* ctx, int64_t n, const float* d_dW, float* d_W, float* d_m, float* d_v,
                                  float alpha, float b1, float b2, float eps, float* d_pow) {
  GAIB_CHECK(ctx && d_pow && ((d_dW && d_W && d_m && d_v) || n == 0), "gaib_adam_step_dev: NULL argument");
  if (n > 0) {
    adam_dev_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, d_dW, d_W, d_m, d_v, alpha, b1, b2, d_pow, eps);
    GAIB_LAUNCH_CHECK();
  }
  adam_advance_kernel<<<1, 1, 0, ctx->stream>>>(d_pow, b1, b2);  // once per call, also for an empty buffer (Q6)
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_gather_rows(gaib_ctx* ctx, int64_t n_idx, const int64_t* d_idx, int len,
                                const float* d_in, float* d_out) {
  GAIB_CHECK(ctx && ((d_idx && d_in && d_out) || n_idx == 0), "gaib_gather_rows: NULL argument");
  if (n_idx <= 0 || len <= 0) return GAIB_OK;
  ProfScope prof(ctx, "gather_rows");
  const bool vec_ok = (len % 4 == 0) && ((((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0);
  if (vec_ok) {
    const int n4 = len / 4;
    int shift = -1;
    for (int b = 0; b < 31; ++b)
      if ((1 << b) == n4) shift = b;
    gather_rows_vec_kernel<0><<<(unsigned)cdiv64(n_idx, 4 * GR_ROWS), 256, 0, ctx->stream>>>(
        n_idx, d_idx, nullptr, n4, shift, reinterpret_cast<const f4*>(d_in), reinterpret_cast<f4*>(d_out));
  } else {
    gather_rows_kernel<<<(unsigned)cdiv64(n_idx, 4), 256, 0, ctx->stream>>>(n_idx, d_idx, len, d_in, d_out);
  }
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// out[dst_idx[k], :] = in[src_idx[k], :]  (see gather_rows_vec_kernel<SCATTER>); dst rows must be distinct
extern "C" int gaib_gather_scatter_rows(gaib_ctx* ctx, int64_t n_idx, const int64_t* d_src_idx, const int64_t* d_dst_idx,
                                        int len, const float* d_in, float* d_out) {
  GAIB_CHECK(ctx && ((d_src_idx && d_dst_idx && d_in && d_out) || n_idx == 0), "gaib_gather_scatter_rows: NULL argument");
  if (n_idx <= 0 || len <= 0) return GAIB_OK;
  ProfScope prof(ctx, "gather_rows");
  const bool vec_ok = (len % 4 == 0) && ((((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0);
  if (vec_ok) {
    const int n4 = len / 4;
    int shift = -1;
    for (int b = 0; b < 31; ++b)
      if ((1 << b) == n4) shift = b;
    gather_rows_vec_kernel<1><<<(unsigned)cdiv64(n_idx, 4 * GR_ROWS), 256, 0, ctx->stream>>>(
        n_idx, d_src_idx, d_dst_idx, n4, shift, reinterpret_cast<const f4*>(d_in), reinterpret_cast<f4*>(d_out));
  } else {
    scatter_rows_kernel<<<(unsigned)cdiv64(n_idx, 4), 256, 0, ctx->stream>>>(n_idx, d_src_idx, d_dst_idx, len, d_in, d_out);
  }
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

// *(float[len]*)d_dst_addr[k] = in[src_idx[k], :]: the source-ordered pack into a send buffer that is several allocations
// (internal: comm.hip).  GAIB_ERR_UNSUPPORTED where the 16-byte path does not apply -- the caller packs chunk by chunk then.
int gaib_gather_rows_to_addresses(gaib_ctx* ctx, int64_t n_idx, const int64_t* d_src_idx, const int64_t* d_dst_addr, int len,
                                  const float* d_in) {
  if (n_idx <= 0 || len <= 0) return GAIB_OK;
  if (len % 4 != 0 || (((uintptr_t)d_in) & 15) != 0) return GAIB_ERR_UNSUPPORTED;  // (chunk bases are 2-MiB aligned, rows 16 B)
  ProfScope prof(ctx, "gather_rows");
  const int n4 = len / 4;
  int shift = -1;
  for (int b = 0; b < 31; ++b)
    if ((1 << b) == n4) shift = b;
  gather_rows_vec_kernel<2><<<(unsigned)cdiv64(n_idx, 4 * GR_ROWS), 256, 0, ctx->stream>>>(
      n_idx, d_src_idx, d_dst_addr, n4, shift, reinterpret_cast<const f4*>(d_in), nullptr);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_bias_add(gaib_ctx* ctx, int64_t n, int len, float* d_x, const float* d_b) {
  GAIB_CHECK(ctx && n >= 0 && len >= 0, "gaib_bias_add: bad argument");
  if (n == 0 || len == 0) return GAIB_OK;
  GAIB_CHECK(d_x && d_b, "gaib_bias_add: NULL pointer");
  GAIB_HIP(hipSetDevice(ctx->device));
  bias_add_kernel<<<stream_grid(n * len, 256), 256, 0, ctx->stream>>>(n * len, len, d_x, d_b);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_colsum(gaib_ctx* ctx, int64_t n, int len, const float* d_x, float* d_a) {
  GAIB_CHECK(ctx && n >= 0 && len >= 0, "gaib_colsum: bad argument");
  if (len == 0) return GAIB_OK;
  GAIB_CHECK(d_a && (d_x || n == 0), "gaib_colsum: NULL pointer");
  GAIB_HIP(hipSetDevice(ctx->device));
  if (n == 0) return gaib_fill_f32(ctx, len, 0.f, d_a);
  int64_t nblocks = (n + 63) / 64;
  if (nblocks > 1024) nblocks = 1024;
  const int64_t rows_per_block = (n + nblocks - 1) / nblocks;
  nblocks = (n + rows_per_block - 1) / rows_per_block;
  GAIB_TRY(gaib_ws_reserve(ctx, sizeof(float) * (size_t)nblocks * (size_t)len));
  colsum_partial_kernel<<<(unsigned)nblocks, 256, 0, ctx->stream>>>(n, len, rows_per_block, d_x, (float*)ctx->ws);
  GAIB_LAUNCH_CHECK();
  colsum_finish_kernel<<<(len + 255) / 256, 256, 0, ctx->stream>>>((int)nblocks, len, (const float*)ctx->ws, d_a);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}

extern "C" int gaib_rng_uniform(gaib_ctx* ctx, int64_t n, float a, float b, uint64_t seed, float* d_r) {
  GAIB_CHECK(ctx && n >= 0 && (d_r || n == 0), "gaib_rng_uniform: bad argument");
  if (n == 0) return GAIB_OK;
  GAIB_HIP(hipSetDevice(ctx->device));
  rng_uniform_kernel<<<stream_grid(n, 256), 256, 0, ctx->stream>>>(n, a, b - a, seed, d_r);
  GAIB_LAUNCH_CHECK();
  return GAIB_OK;
}
