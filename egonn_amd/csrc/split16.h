// The project's fp16 split arithmetic (gfx950), stated once for every consumer: the sparse convolutions of sconv_split.hip, the
// SPLIT instantiation of sconv.hip, the top-down step of topdown.hip and the local heads of heads.hip.  Device helpers only.
//
// Why.  v_mfma_f32_16x16x4_f32 runs at the fp32 VECTOR rate (157 TFLOP/s, 1/16 of the 16-bit matrix rate) and was the binding
// roof of every fp32 layer with >= 64 channels.  Round 3 ran these layers on v_mfma_f32_16x16x32_bf16 with
// both operands split EXACTLY into three bf16 parts and six products; the kernels then turned out to be bound by their own
// instruction stream (44 of 68 vector instructions per group and step were the split, profiles/r03c_pmc_wide.txt).  Round 5: fp16 parts.
// An fp16 number carries 11 significand bits, so  x = hi + lo + r  with hi = rn16(x), lo = rn16(x - hi), |r| <= 2^-22 |x|
// (fp32 itself rounds at 2^-24), an fp16 x fp16 product is exact in fp32, and
//     a * w = ah*wh + ah*wl + al*wh  (+ al*wl + cross terms with r: <= 3 * 2^-22 |a w|, dropped)
// is THREE products on v_mfma_f32_16x16x32_f16 (same rate as bf16) instead of six, a 24-instruction split instead of 44, and
// 4 bytes per weight instead of 6.  Range: fp16 holds |x| < 65504.  Weights are scaled by a power of two per kernel at pack
// time (max |W| -> [2^13, 2^14); exact, undone exactly in the epilogue) so that their low parts stay normal numbers;
// activations are used as they are: an fp32 activation beyond +-65504 becomes Inf in the split — every accumulator that gathers it
// then is Inf / NaN and the epilogue raises the plan's range flag (split_raise; egonn_plan_status: EGONN_STATUS_FP16_RANGE;
// egonn_ctx_set_exact_fp32 selects the exact kernels of sconv.hip) — and the low part of an activation below 2^-3 is a subnormal
// with an ABSOLUTE error <= 2^-25: nothing next to the rounding of the sums these layers produce (operands far below 1 — input
// gradients — are scaled per launch: SplitArgs::in_maxbits).  Measured against the plain fp32 kernel
// (tests/test_gpu_graph.py::test_split_conv_matches_exact_fp32, tests/test_gpu_range.py): DESIGN.md §3.1.
//
// The project promises the same bits on every route (pre-split maps vs the in-loop split, resident vs lock-step, fused vs unfused)
// and one meaning of the range flag: both hold because every route takes its split, its term order and its guard from here.
#pragma once
#include "common.h"

namespace egonn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

// fp16 parts hold |x| < 65520: 65504 <= |x| < 65520 rounds to 65504 with an exact low part, |x| >= 65520 to Inf
constexpr float SPLIT_FP16_LIMIT = 65520.f;

// channel of the 32-channel block that lane group g (= lane >> 4) holds in element e of its 8-element MFMA operand: the two
// 16-byte chunks g and 4+g of a 128-byte row (the conflict-free ds_read_b128 pattern of the swizzled image)
__host__ __device__ static inline int split_chan(int g, int e) { return e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4); }

// fp32 x 8 -> (hi, lo) fp16 x 8, round to nearest even at both levels (v_cvt_pk_f16_f32): 24 VALU
__device__ static inline void split8h(const f32x4& a0, const f32x4& a1, f16x8_t& hi, f16x8_t& lo) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float x0 = p < 2 ? a0[2 * p] : a1[2 * p - 4], x1 = p < 2 ? a0[2 * p + 1] : a1[2 * p - 3];
    const f16x2_t h = __builtin_convertvector((f32x2){x0, x1}, f16x2_t);
    const f32x2 hf = __builtin_convertvector(h, f32x2);
    const f16x2_t l = __builtin_convertvector((f32x2){x0 - hf[0], x1 - hf[1]}, f16x2_t);
    hi[2 * p] = h[0]; hi[2 * p + 1] = h[1];
    lo[2 * p] = l[0]; lo[2 * p + 1] = l[1];
  }
}

// ------------------------------------------------------------------ packs: weights scaled by a power of two, hi | lo fragments
// this thread's share of max |w[i]| over the finite elements, i = start, start + stride, ... < n (NaN / Inf do not pick the
// scale), reduced over the 64 lanes of its wave; the caller's lane 0 of every wave does the atomicMax on the bits
template <typename I, typename S>
__device__ static inline float split_finite_absmax(const float* __restrict__ w, I n, I start, S stride) {
  float m = 0.f;
  for (I i = start; i < n; i += stride) {
    const float v = fabsf(w[i]);
    m = (v == v && v < INFINITY) ? fmaxf(m, v) : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}
__device__ static inline float split_scale_of(uint32_t maxbits) {     // power of two s with s * max in [2^13, 2^14)
  const int e = (int)(maxbits >> 23) - 127;                            // max = 1.m * 2^e (0 / subnormal: e = -127 -> clamped)
  const int se = min(max(13 - e, -100), 100);
  return __uint_as_float((uint32_t)(se + 127) << 23);
}
__device__ static inline _Float16 split_part(float v, int part) {      // hi (part 0) or lo (part 1) of an already scaled weight
  const _Float16 hi = (_Float16)v;
  const _Float16 lo = (_Float16)(v - (float)hi);
  return part == 0 ? hi : lo;
}
// A pack (pack_split_weights) is [fragments | float 1/s | uint32 bits of max |W| | pad]: a 16-byte trailer behind 4 bytes per weight
__host__ __device__ constexpr size_t split_frag_bytes(int K, int cin, int cout) { return (size_t)K * cin * cout * 4; }
constexpr size_t SPLIT_TRAILER_BYTES = 16;
__device__ static inline float split_pack_winv(const void* pack, size_t frag_bytes) {   // 1 / (pack scale): a power of two
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(pack) + frag_bytes);
}
__device__ static inline float split_pack_winv(const void* pack, int K, int cin, int cout) {
  return split_pack_winv(pack, split_frag_bytes(K, cin, cout));
}

// ------------------------------------------------------------------ the three products, small terms first
// THE ORDER: w_lo * a_hi, then w_hi * a_lo, then w_hi * a_hi, on one fp32 accumulator (weights are the MFMA's A operand: D^T = W^T A^T)
__device__ static inline void split_mfma3(const f16x8_t& wh, const f16x8_t& wl, const f16x8_t& ah, const f16x8_t& al, f32x4& acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, ah, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, al, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, ah, acc, 0, 0, 0);
}
// the two column tiles of a 32-column slice against the same rows: the same order per accumulator, the tiles interleaved term by
// term (lo0 lo1 / hi*al0 hi*al1 / hh0 hh1) so that no MFMA waits for the one in front of it
__device__ static inline void split_mfma3(const f16x8_t& wh0, const f16x8_t& wh1, const f16x8_t& wl0, const f16x8_t& wl1,
                                          const f16x8_t& ah, const f16x8_t& al, f32x4& acc0, f32x4& acc1) {
  acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl0, ah, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl1, ah, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh0, al, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh1, al, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh0, ah, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh1, ah, acc1, 0, 0, 0);
}

// ------------------------------------------------------------------ range guard
// (x - x) is 0 for finite x and NaN for Inf / NaN, and NaN is sticky under addition: the probes of many values are summed and
// tested once (!= 0).  An epilogue probes every accumulator before BN / ReLU can hide it and raises the plan's range bit
// (common.h: SPLIT_RANGE_BIT) — the flag says "this launch's fp32 semantics are not guaranteed".
__device__ static inline float split_nonfinite(float v) { return v - v; }
__device__ static inline float split_nonfinite(f32x4 v) {
  const f32x4 z = v - v;
  return (z[0] + z[1]) + (z[2] + z[3]);
}
__device__ static inline float split_nonfinite(f32x4 a, f32x4 b) {       // two tiles, one horizontal sum
  const f32x4 z = (a - a) + (b - b);
  return (z[0] + z[1]) + (z[2] + z[3]);
}
__device__ static inline void split_raise(int32_t* flags) { atomicOr(flags, SPLIT_RANGE_BIT); }

}  // namespace egonn
