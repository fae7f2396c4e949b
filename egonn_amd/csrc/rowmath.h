// Device helpers shared by the translation units that work on rows of feature maps: the activation of an epilogue, the
// bf16 <-> fp32 conversions of bf16 feature maps, the scan of a row and the sum over the 16 rows of an accumulator tile.
// Defined once, here (f32x4 and the other vector types: split16.h).
#pragma once
#include "common.h"
#include "kernels.h"
#include "split16.h"

namespace egonn {

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

__device__ static inline float row16_sum(float v) {      // sum over the 16 lanes of a DPP row (= the 16 rows of a tile)
  int x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
  x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
  x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true));   // row_half_mirror
  x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true));   // row_mirror
  return v;
}

}  // namespace egonn
