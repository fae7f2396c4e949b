// Device helpers shared by the row-wise translation units (dense.hip, rowwise.hip, heads.hip): the activation of an epilogue,
// the bf16 <-> fp32 conversions of bf16 feature maps and the scan of a row.  Defined once, here.
#pragma once
#include "common.h"
#include "kernels.h"

namespace egonn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ static inline float apply_act(float v, int act) {
  switch (act) {
    case ACT_RELU: return fmaxf(v, 0.f);
    case ACT_TANH: return tanhf(v);
    case ACT_SOFTPLUS: return v > 20.f ? v : log1pf(expf(v));     // torch softplus(beta=1, threshold=20)
    case ACT_SIGMOID: return 1.f / (1.f + expf(-v));
    default: return v;
  }
}

// bf16 feature maps (configs[2]): widened exactly to fp32 in registers, rounded to nearest even on the way out
__device__ static inline float bf2f(uint32_t h) { return __uint_as_float(h << 16); }
__device__ static inline uint32_t f2bf_rn(float a) {
  uint32_t u = __float_as_uint(a);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}

// sample (scan) of row r: last b with boff[b] <= r
__device__ static inline int sample_of_row(const int32_t* __restrict__ boff, int B, int32_t r) {
  int lo = 0, hi = B;   // boff[lo] <= r < boff[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (boff[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace egonn
