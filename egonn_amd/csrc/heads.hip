// The local heads of EgoNN: keypoint positions, the descriptor decoder / keypoint regressor / sigma regressor in one launch
// (exact fp32 and fp16-split forms, with the packer of the latter) and top-k keypoint selection.
//
// Reference call sites: Quantizer.keypoint_position datasets/quantization.py:60-72,93-103 ; the heads models/minkgl.py:175-225,287-308 ;
// torch.topk eval/evaluate.py:359.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "rowmath.h"
#include "split16.h"

namespace egonn {

// ------------------------------------------------------------------ keypoint positions
// Quantizer.keypoint_position (datasets/quantization.py:60-72 polar, 93-103 Cartesian) of one super-voxel
__device__ static inline void keypoint_position(uint64_t key, int level, int cb, float ox, float oy, float oz, int mode,
                                                float s0, float s1, float s2, float* __restrict__ out3) {
  const int cbL = cb - level;
  const uint64_t mort = key & ((1ull << (3 * cbL)) - 1);
  const int32_t bias = 1 << (cb - 1);
  const float cx = (float)(((int32_t)compact1by2(mort) << level) - bias);
  const float cy = (float)(((int32_t)compact1by2(mort >> 1) << level) - bias);
  const float cz = (float)(((int32_t)compact1by2(mort >> 2) << level) - bias);
  const float stride = (float)(1 << level);
  // (C + 0.5) * q + offset * (stride * q) / 2, evaluated like the reference (no contraction)
  const float px = __fadd_rn(__fmul_rn(__fadd_rn(cx, 0.5f), s0), __fdiv_rn(__fmul_rn(ox, __fmul_rn(stride, s0)), 2.f));
  const float py = __fadd_rn(__fmul_rn(__fadd_rn(cy, 0.5f), s1), __fdiv_rn(__fmul_rn(oy, __fmul_rn(stride, s1)), 2.f));
  const float pz = __fadd_rn(__fmul_rn(__fadd_rn(cz, 0.5f), s2), __fdiv_rn(__fmul_rn(oz, __fmul_rn(stride, s2)), 2.f));
  if (mode == 0) {
    out3[0] = px; out3[1] = py; out3[2] = pz;
  } else {
    // polar -> cartesian (reference quantization.py:46-53): theta = pi * (deg - 180) / 180
    const float theta = __fdiv_rn(__fmul_rn(3.14159265358979323846f, __fadd_rn(px, -180.f)), 180.f);
    out3[0] = cosf(theta) * py;
    out3[1] = sinf(theta) * py;
    out3[2] = pz;
  }
}

__global__ void keypoint_kernel(const uint64_t* __restrict__ keys, int64_t n, int level, int cb,
                                const float* __restrict__ offs, int mode, float s0, float s1, float s2, int ignore,
                                float* __restrict__ out, const int32_t* __restrict__ n_dev) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n_dev) n = min((int64_t)*n_dev, n);
  if (i >= n) return;
  const float kox = ignore ? 0.f : offs[3 * i + 0], koy = ignore ? 0.f : offs[3 * i + 1],
              koz = ignore ? 0.f : offs[3 * i + 2];
  keypoint_position(keys[i], level, cb, kox, koy, koz, mode, s0, s1, s2, out + 3 * i);
}
int keypoint_positions(const uint64_t* keys, int64_t n, int level, int cb, const float* offsets, int mode,
                       const float* step, int ignore_offsets, float* out, hipStream_t stream, const int32_t* n_dev) {
  if (n == 0) return EGONN_OK;
  const float s0 = step[0], s1 = mode ? step[1] : step[0], s2 = mode ? step[2] : step[0];
  hipLaunchKernelGGL(keypoint_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, keys, n, level, cb, offsets,
                     mode, s0, s1, s2, ignore_offsets, out, n_dev);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ the three local heads in one launch
// DescriptorDecoder (Linear 64->96, ReLU, Linear 96->128, L2 normalise), KeypointRegressor (64->32, ReLU, 32->3, tanh,
// Quantizer.keypoint_position) and SigmaRegressor (64->32, ReLU, 32->1, softplus) of models/minkgl.py:175-225,287-308
// read the local feature map ONCE.  A wave owns 16 rows; operands are fed swapped (D^T = W^T X^T), so a lane ends up with
// four consecutive hidden units of its row — exactly the B fragment of the next layer's MFMA (contraction index
// 16t + 4g + u), i.e. the MLPs chain in registers.  Weights are read in nn.Linear (out,in) layout, one float4 per lane.
struct LocalHeadsArgs {
  const float* x;                                          // (n, 64)
  const float *lw, *lres;                                  // non-null: the head's lateral 1x1 convolution runs here first —
                                                           // x := x @ lw + lres (lw (64,64) in (cin, cout) layout, lres (n,64))
  const float *dw0, *db0, *dw1, *db1;                      // descriptor decoder: (96,64),(96),(128,96),(128)
  const float *kw0, *kb0, *kw1, *kb1;                      // keypoint regressor: (32,64),(32),(3,32),(3)
  const float *sw0, *sb0, *sw1, *sb1;                      // sigma regressor:    (32,64),(32),(1,32),(1)
  const uint64_t* keys;                                    // level-3 keys (super-voxel coordinates)
  const int32_t* n_dev;                                    // device row count (nullable)
  float *out_desc, *out_kp, *out_sigma;
  int64_t n;
  int level, cb, mode, ignore_offsets;
  int in_bf16;                                             // x and lres are bf16 maps (bf16 feature maps; only with lw)
  float s0, s1, s2;
};
// The six weight matrices (92 KB as MFMA fragments) are staged ONCE per workgroup into LDS in fragment order
//   frag[(nt * CIN/16 + t) * 64 + lane] = W[16 nt + (lane & 15)][16 t + 4 (lane >> 4) .. +3]      (rows >= rows_w: zeros)
// so that a wave's B operands are lane-linear ds_read_b128 (conflict-free) instead of 92 KB of dependent global loads per
// 16-row tile — the first version spent 60 us on 1.4 GFLOP because every wave re-fetched every weight through L1.
template <int CIN, int NT>
__device__ static inline void stage_frags(const float* __restrict__ W, int rows_w, f32x4* __restrict__ dst, int tid, int nthreads) {
  constexpr int T = CIN / 16;
  for (int i = tid; i < NT * T * 64; i += nthreads) {
    const int lane = i & 63, ft = i >> 6;
    const int nt = ft / T, t = ft - nt * T;
    const int unit = 16 * nt + (lane & 15);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (unit < rows_w) v = *reinterpret_cast<const f32x4*>(W + (int64_t)unit * CIN + 16 * t + 4 * (lane >> 4));
    dst[i] = v;
  }
}
template <int CIN, int NT>   // out[nt] = sum_k W[16nt + l15][k] * in[k]  for the 16 rows of the wave (swapped operands)
__device__ static inline void mlp_layer(const f32x4* __restrict__ frags, const f32x4* __restrict__ in, int lane,
                                        f32x4* __restrict__ out) {
  constexpr int T = CIN / 16;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const f32x4 wf = frags[(nt * T + t) * 64 + lane];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[u], in[t][u], acc, 0, 0, 0);
    }
    out[nt] = acc;
    __builtin_amdgcn_sched_barrier(0);                   // keep the fragment reads of later tiles from being hoisted (spills)
  }
}
// the same staging for a (cin, cout)-layout matrix (1x1 convolution kernels): frag = W[16 t + 4 (lane >> 4) .. +3][16 nt + (lane & 15)]
template <int CIN, int NT>
__device__ static inline void stage_frags_t(const float* __restrict__ W, int cout, f32x4* __restrict__ dst, int tid, int nthreads) {
  constexpr int T = CIN / 16;
  for (int i = tid; i < NT * T * 64; i += nthreads) {
    const int lane = i & 63, ft = i >> 6;
    const int nt = ft / T, t = ft - nt * T;
    const float* wp = W + (int64_t)(16 * t + 4 * (lane >> 4)) * cout + 16 * nt + (lane & 15);
    dst[i] = (f32x4){wp[0], wp[cout], wp[2 * (int64_t)cout], wp[3 * (int64_t)cout]};
  }
}
constexpr int LH_F_DW0 = 0, LH_F_DW1 = LH_F_DW0 + 6 * 4, LH_F_KW0 = LH_F_DW1 + 8 * 6, LH_F_KW1 = LH_F_KW0 + 2 * 4,
              LH_F_SW0 = LH_F_KW1 + 1 * 2, LH_F_SW1 = LH_F_SW0 + 2 * 4, LH_FRAGS = LH_F_SW1 + 1 * 2;      // 92 fragments of 1 KB
__global__ __launch_bounds__(LH_WAVES * 64) void local_heads_kernel(const LocalHeadsArgs p) {
  extern __shared__ __attribute__((aligned(16))) f32x4 lh_frags[];      // [LH_FRAGS][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g4 = lane >> 4;
  stage_frags<64, 6>(p.dw0, 96, lh_frags + LH_F_DW0 * 64, tid, LH_WAVES * 64);
  stage_frags<96, 8>(p.dw1, 128, lh_frags + LH_F_DW1 * 64, tid, LH_WAVES * 64);
  stage_frags<64, 2>(p.kw0, 32, lh_frags + LH_F_KW0 * 64, tid, LH_WAVES * 64);
  stage_frags<32, 1>(p.kw1, 3, lh_frags + LH_F_KW1 * 64, tid, LH_WAVES * 64);
  stage_frags<64, 2>(p.sw0, 32, lh_frags + LH_F_SW0 * 64, tid, LH_WAVES * 64);
  stage_frags<32, 1>(p.sw1, 1, lh_frags + LH_F_SW1 * 64, tid, LH_WAVES * 64);
  if (p.lw) stage_frags_t<64, 4>(p.lw, 64, lh_frags + LH_FRAGS * 64, tid, LH_WAVES * 64);
  __syncthreads();
  int64_t n = p.n;
  if (p.n_dev) n = min((int64_t)*p.n_dev, n);
  const int64_t ntiles = (n + 15) >> 4;
  for (int64_t tile = (int64_t)blockIdx.x * LH_WAVES + wave; tile < ntiles; tile += (int64_t)gridDim.x * LH_WAVES) {
    const int64_t row = tile * 16 + l15;
    const bool ok = row < n;
    f32x4 x[4];
    auto load4 = [&](const float* base, int t) -> f32x4 {     // four channels of the row: fp32, or bf16 widened
      if (!ok) return (f32x4){0.f, 0.f, 0.f, 0.f};
      if (p.in_bf16) {
        const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(base) + row * 64 + 16 * t + 4 * g4);
        return (f32x4){bf2f(h.x & 0xFFFFu), bf2f(h.x >> 16), bf2f(h.y & 0xFFFFu), bf2f(h.y >> 16)};
      }
      return *reinterpret_cast<const f32x4*>(base + row * 64 + 16 * t + 4 * g4);
    };
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = load4(p.x, t);
    if (p.lw) {
      // ---- MinkHead's last lateral (models/minkgl.py:46-60): conv1x1(x3) + the transposed convolution's output, in the
      //      accumulation order of the dense kernel it replaces (bitwise the same rows); the 64-channel map the three heads read
      //      never goes to memory
      f32x4 r[4], l[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) r[t] = load4(p.lres, t);
      mlp_layer<64, 4>(lh_frags + LH_FRAGS * 64, x, lane, l);
#pragma unroll
      for (int t = 0; t < 4; ++t) x[t] = l[t] + r[t];
    }
    // ---- descriptor decoder + L2 normalisation
    {
      f32x4 h[6], o[8];
      mlp_layer<64, 6>(lh_frags + LH_F_DW0 * 64, x, lane, h);
#pragma unroll
      for (int nt = 0; nt < 6; ++nt) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.db0 + 16 * nt + 4 * g4);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[nt][r] = fmaxf(h[nt][r] + b[r], 0.f);
      }
      mlp_layer<96, 8>(lh_frags + LH_F_DW1 * 64, h, lane, o);
      float ss = 0.f;
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.db1 + 16 * nt + 4 * g4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          o[nt][r] += b[r];
          ss += o[nt][r] * o[nt][r];
        }
      }
      ss += __shfl_xor(ss, 16, 64);
      ss += __shfl_xor(ss, 32, 64);
      const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);      // F.normalize(p=2, dim=1, eps=1e-12)
      if (ok) {
#pragma unroll
        for (int nt = 0; nt < 8; ++nt)
          *reinterpret_cast<f32x4*>(p.out_desc + row * 128 + 16 * nt + 4 * g4) = o[nt] * inv;
      }
    }
    // ---- keypoint regressor -> position of the keypoint in metres
    {
      f32x4 h[2], o[1];
      mlp_layer<64, 2>(lh_frags + LH_F_KW0 * 64, x, lane, h);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.kb0 + 16 * nt + 4 * g4);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[nt][r] = fmaxf(h[nt][r] + b[r], 0.f);
      }
      mlp_layer<32, 1>(lh_frags + LH_F_KW1 * 64, h, lane, o);
      if (ok && g4 == 0) {                                   // lane (row, g = 0) holds output units 0..3
        const float ox = p.ignore_offsets ? 0.f : tanhf(o[0][0] + p.kb1[0]);
        const float oy = p.ignore_offsets ? 0.f : tanhf(o[0][1] + p.kb1[1]);
        const float oz = p.ignore_offsets ? 0.f : tanhf(o[0][2] + p.kb1[2]);
        keypoint_position(p.keys[row], p.level, p.cb, ox, oy, oz, p.mode, p.s0, p.s1, p.s2, p.out_kp + row * 3);
      }
    }
    // ---- sigma regressor
    {
      f32x4 h[2], o[1];
      mlp_layer<64, 2>(lh_frags + LH_F_SW0 * 64, x, lane, h);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.sb0 + 16 * nt + 4 * g4);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[nt][r] = fmaxf(h[nt][r] + b[r], 0.f);
      }
      mlp_layer<32, 1>(lh_frags + LH_F_SW1 * 64, h, lane, o);
      if (ok && g4 == 0) p.out_sigma[row] = apply_act(o[0][0] + p.sb1[0], ACT_SOFTPLUS);
    }
  }
}
// ------------------------------------------------------------------ the three heads on the fp16 matrix pipe (round 6)
// local_heads_kernel above is bound by v_mfma_f32_16x16x4_f32: 432 MFMAs of 32 cycles per 16-row tile, two waves per SIMD —
// 1 831 tiles x 13.8 k cycles / 1 024 SIMDs = 10 us of the 36 us launch at best.  The heads' six Linear layers here run with
// the two-way fp16 split of split16.h instead (weights packed ONCE per model as hi | lo fragments in the contraction
// order of the register chain, one power-of-two scale per matrix; activations split in registers; three products on
// v_mfma_f32_16x16x32_f16, small terms first): 138 MFMAs of 16 cycles.  The lateral 1x1 convolution in front stays on the exact
// pipe in the accumulation order of the dense kernel (the fused / unfused switch stays bitwise).  Deviation of the outputs from
// the exact kernel: < 3e-6 of the largest value per output (tests/test_gpu_fusions.py).  Range guard (the plan's fp16 range flag):
// the heads' input tile (lateral + transposed convolution, exact fp32) is tested for |x| >= SPLIT_FP16_LIMIT and non-finite elements before it
// is split — the first layers' ReLU would otherwise turn the NaN accumulators of such an input into 0 — and the outputs of the
// second layers for non-finite values (a hidden activation beyond the range).  egonn_ctx_set_exact_fp32 selects the kernel above.
// fragments (1 KB hi + 1 KB lo each) per matrix: NT * CIN / 32
constexpr int LHS_DW0 = 0, LHS_DW1 = LHS_DW0 + 6 * 2, LHS_KW0 = LHS_DW1 + 8 * 3, LHS_KW1 = LHS_KW0 + 2 * 2, LHS_SW0 = LHS_KW1 + 1 * 1,
              LHS_SW1 = LHS_SW0 + 2 * 2, LHS_FRAGS = LHS_SW1 + 1 * 1;                                   // 46 fragment pairs = 92 KB
struct LhsMat { int cin, nout, nt, first; };
__constant__ LhsMat lhs_mats[6] = {{64, 96, 6, LHS_DW0}, {96, 128, 8, LHS_DW1}, {64, 32, 2, LHS_KW0}, {32, 3, 1, LHS_KW1},
                                   {64, 32, 2, LHS_SW0}, {32, 1, 1, LHS_SW1}};
__global__ void lhs_absmax_kernel(const float* const* __restrict__ W, uint32_t* __restrict__ trailer) {
  const int mi = blockIdx.x;
  const LhsMat M = lhs_mats[mi];
  const float* w = W[mi];
  const float m = split_finite_absmax(w, M.cin * M.nout, (int)threadIdx.x, blockDim.x);
  if ((threadIdx.x & 63) == 0) atomicMax(trailer + 8 + mi, __float_as_uint(m));
}
// out[(first + nt * KB + kb) * 2 + part][lane][e] = part(s * W[16 nt + (lane & 15)][32 kb + split_chan(lane >> 4, e)]) (fp16),
// rows beyond nout: zeros; behind the fragments: float 1/s per matrix [0..5], max bits [8..13]
__global__ void lhs_pack_kernel(const float* const* __restrict__ W, uint16_t* __restrict__ out, uint32_t* __restrict__ trailer) {
  const int mi = blockIdx.y;
  const LhsMat M = lhs_mats[mi];
  const int KB = M.cin / 32;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const float sc = split_scale_of(trailer[8 + mi]);
  if (t == 0) reinterpret_cast<float*>(trailer)[mi] = 1.f / sc;
  if (t >= M.nt * KB * 2 * 64 * 8) return;
  int r = t;
  const int e = r & 7; r >>= 3;
  const int lane = r & 63; r >>= 6;
  const int part = r & 1; r >>= 1;
  const int kb = r % KB, nt = r / KB;
  const int unit = 16 * nt + (lane & 15), k = 32 * kb + split_chan(lane >> 4, e);
  const float v = unit < M.nout ? sc * W[mi][(int64_t)unit * M.cin + k] : 0.f;
  out[(int64_t)M.first * 2 * 512 + t] = __builtin_bit_cast(uint16_t, split_part(v, part));
}
size_t local_heads_pack_bytes() { return (size_t)LHS_FRAGS * 2048 + 64; }
int local_heads_pack(const float* const* w6_dev /*device array of the six weight pointers*/, void* out, hipStream_t stream) {
  uint32_t* trailer = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(out) + (size_t)LHS_FRAGS * 2048);
  HIP_CHECK(hipMemsetAsync(trailer, 0, 64, stream));
  hipLaunchKernelGGL(lhs_absmax_kernel, dim3(6), dim3(256), 0, stream, w6_dev, trailer);
  hipLaunchKernelGGL(lhs_pack_kernel, dim3((8 * 3 * 2 * 64 * 8 + 255) / 256, 6), dim3(256), 0, stream, w6_dev,
                     reinterpret_cast<uint16_t*>(out), trailer);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
// out[nt] = winv * sum_kb (W_lo ah + W_hi al + W_hi ah): in = f32x4 per 16 input channels (the register chain's layout)
template <int CIN, int NT>
__device__ static inline void lhs_layer(const f32x4* __restrict__ frags /* pairs: hi, lo */, const f32x4* __restrict__ in, int lane,
                                        float winv, f32x4* __restrict__ out) {
  constexpr int KB = CIN / 32;
  f16x8_t ah[KB], al[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) split8h(in[2 * kb], in[2 * kb + 1], ah[kb], al[kb]);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const f16x8_t wh = __builtin_bit_cast(f16x8_t, frags[((nt * KB + kb) * 2) * 64 + lane]);
      const f16x8_t wl = __builtin_bit_cast(f16x8_t, frags[((nt * KB + kb) * 2 + 1) * 64 + lane]);
      split_mfma3(wh, wl, ah[kb], al[kb], acc);
    }
    out[nt] = acc * winv;
    __builtin_amdgcn_sched_barrier(0);
  }
}
struct LocalHeadsSplitArgs {
  LocalHeadsArgs a;
  const void* pack;          // local_heads_pack
  int32_t* flags;            // the plan's flag word (split_raise: input beyond the fp16 range, non-finite head output)
};
__global__ __launch_bounds__(LH_WAVES * 64) void local_heads_split_kernel(const LocalHeadsSplitArgs q) {
  const LocalHeadsArgs& p = q.a;
  extern __shared__ __attribute__((aligned(16))) f32x4 lh_frags[];      // [LHS_FRAGS * 2][64] split fragments, then the lateral's 16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g4 = lane >> 4;
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(q.pack);
    for (int i = tid; i < LHS_FRAGS * 2 * 64; i += LH_WAVES * 64) lh_frags[i] = src[i];
  }
  f32x4* const lat = lh_frags + LHS_FRAGS * 2 * 64;
  if (p.lw) stage_frags_t<64, 4>(p.lw, 64, lat, tid, LH_WAVES * 64);
  const float* winv = reinterpret_cast<const float*>(reinterpret_cast<const char*>(q.pack) + (size_t)LHS_FRAGS * 2048);
  const float wi0 = winv[0], wi1 = winv[1], wi2 = winv[2], wi3 = winv[3], wi4 = winv[4], wi5 = winv[5];
  __syncthreads();
  int64_t n = p.n;
  if (p.n_dev) n = min((int64_t)*p.n_dev, n);
  const int64_t ntiles = (n + 15) >> 4;
  for (int64_t tile = (int64_t)blockIdx.x * LH_WAVES + wave; tile < ntiles; tile += (int64_t)gridDim.x * LH_WAVES) {
    const int64_t row = tile * 16 + l15;
    const bool ok = row < n;
    f32x4 x[4];
    auto load4 = [&](const float* base, int t) -> f32x4 {
      if (!ok) return (f32x4){0.f, 0.f, 0.f, 0.f};
      if (p.in_bf16) {
        const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(base) + row * 64 + 16 * t + 4 * g4);
        return (f32x4){bf2f(h.x & 0xFFFFu), bf2f(h.x >> 16), bf2f(h.y & 0xFFFFu), bf2f(h.y >> 16)};
      }
      return *reinterpret_cast<const f32x4*>(base + row * 64 + 16 * t + 4 * g4);
    };
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = load4(p.x, t);
    if (p.lw) {                                              // the lateral: exact pipe, the dense kernel's order (bitwise)
      f32x4 r[4], l[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) r[t] = load4(p.lres, t);
      mlp_layer<64, 4>(lat, x, lane, l);
#pragma unroll
      for (int t = 0; t < 4; ++t) x[t] = l[t] + r[t];
    }
    float guard = 0.f;                                       // sum of split_nonfinite probes
    // the heads' input (fp32, or bf16 widened): an element fp16 cannot hold (|x| >= SPLIT_FP16_LIMIT rounds to Inf; below it to
    // a finite hi with an exact low part) or a non-finite one turns the first layers' accumulators into NaN, which the bias + ReLU
    // below (fmaxf) would turn into 0 — so the input tile itself is checked, before any of it enters the split
    bool outside = false;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) outside |= !(fabsf(x[t][r]) < SPLIT_FP16_LIMIT);
    // ---- descriptor decoder + L2 normalisation
    {
      f32x4 h[6], o[8];
      lhs_layer<64, 6>(lh_frags + LHS_DW0 * 2 * 64, x, lane, wi0, h);
#pragma unroll
      for (int nt = 0; nt < 6; ++nt) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.db0 + 16 * nt + 4 * g4);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[nt][r] = fmaxf(h[nt][r] + b[r], 0.f);
      }
      lhs_layer<96, 8>(lh_frags + LHS_DW1 * 2 * 64, h, lane, wi1, o);
      float ss = 0.f;
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.db1 + 16 * nt + 4 * g4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          o[nt][r] += b[r];
          ss += o[nt][r] * o[nt][r];
        }
      }
      ss += __shfl_xor(ss, 16, 64);
      ss += __shfl_xor(ss, 32, 64);
      guard += split_nonfinite(ss);
      const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
      if (ok) {
#pragma unroll
        for (int nt = 0; nt < 8; ++nt)
          *reinterpret_cast<f32x4*>(p.out_desc + row * 128 + 16 * nt + 4 * g4) = o[nt] * inv;
      }
    }
    // ---- keypoint regressor -> position of the keypoint in metres
    {
      f32x4 h[2], o[1];
      lhs_layer<64, 2>(lh_frags + LHS_KW0 * 2 * 64, x, lane, wi2, h);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.kb0 + 16 * nt + 4 * g4);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[nt][r] = fmaxf(h[nt][r] + b[r], 0.f);
      }
      lhs_layer<32, 1>(lh_frags + LHS_KW1 * 2 * 64, h, lane, wi3, o);
      if (ok && g4 == 0) {
        guard += split_nonfinite(o[0][0]) + split_nonfinite(o[0][1]) + split_nonfinite(o[0][2]);
        const float ox = p.ignore_offsets ? 0.f : tanhf(o[0][0] + p.kb1[0]);
        const float oy = p.ignore_offsets ? 0.f : tanhf(o[0][1] + p.kb1[1]);
        const float oz = p.ignore_offsets ? 0.f : tanhf(o[0][2] + p.kb1[2]);
        keypoint_position(p.keys[row], p.level, p.cb, ox, oy, oz, p.mode, p.s0, p.s1, p.s2, p.out_kp + row * 3);
      }
    }
    // ---- sigma regressor
    {
      f32x4 h[2], o[1];
      lhs_layer<64, 2>(lh_frags + LHS_SW0 * 2 * 64, x, lane, wi4, h);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.sb0 + 16 * nt + 4 * g4);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[nt][r] = fmaxf(h[nt][r] + b[r], 0.f);
      }
      lhs_layer<32, 1>(lh_frags + LHS_SW1 * 2 * 64, h, lane, wi5, o);
      if (ok && g4 == 0) {
        guard += split_nonfinite(o[0][0]);
        p.out_sigma[row] = apply_act(o[0][0] + p.sb1[0], ACT_SOFTPLUS);
      }
    }
    if (ok && (outside || guard != 0.f) && q.flags) split_raise(q.flags);
  }
}

int local_heads_forward(const float* x, int64_t n, const int32_t* n_dev, const float* const* w /*12 pointers*/,
                        const uint64_t* keys, int level, int cb, int mode, const float* step, int ignore_offsets,
                        float* out_desc, float* out_kp, float* out_sigma, hipStream_t stream, const float* lateral_w,
                        const float* lateral_res, int in_bf16, const void* split_pack, int32_t* flags) {
  if (n == 0) return EGONN_OK;
  EGONN_REQUIRE((lateral_w == nullptr) == (lateral_res == nullptr), EGONN_ERR_INVALID, "local heads: lateral kernel and residual go together");
  LocalHeadsArgs a;
  a.x = x; a.n = n; a.n_dev = n_dev;
  a.lw = lateral_w; a.lres = lateral_res;
  a.in_bf16 = in_bf16 ? 1 : 0;
  EGONN_REQUIRE(!in_bf16 || lateral_w, EGONN_ERR_INVALID, "local heads: bf16 input rows only through the fused lateral");
  a.dw0 = w[0]; a.db0 = w[1]; a.dw1 = w[2]; a.db1 = w[3];
  a.kw0 = w[4]; a.kb0 = w[5]; a.kw1 = w[6]; a.kb1 = w[7];
  a.sw0 = w[8]; a.sb0 = w[9]; a.sw1 = w[10]; a.sb1 = w[11];
  a.keys = keys; a.level = level; a.cb = cb; a.mode = mode; a.ignore_offsets = ignore_offsets;
  a.s0 = step[0]; a.s1 = mode ? step[1] : step[0]; a.s2 = mode ? step[2] : step[0];
  a.out_desc = out_desc; a.out_kp = out_kp; a.out_sigma = out_sigma;
  const int64_t tiles = cdiv(n, 16);
  const size_t lds = (size_t)(LH_FRAGS + (lateral_w ? 16 : 0)) * 64 * sizeof(f32x4);
  static AttrOnce attr_done;
  if (attr_done.need()) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&local_heads_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_done.mark(); 
  }
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(tiles, LH_WAVES), 256);      // one workgroup per CU holds the weights
  if (split_pack) {
    static AttrOnce attr2;
    if (attr2.need()) {
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&local_heads_split_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr2.mark();
    }
    LocalHeadsSplitArgs q;
    q.a = a; q.pack = split_pack; q.flags = flags;
    const size_t lds2 = (size_t)(LHS_FRAGS * 2 + (lateral_w ? 16 : 0)) * 64 * sizeof(f32x4);
    hipLaunchKernelGGL(local_heads_split_kernel, dim3(grid), dim3(LH_WAVES * 64), lds2, stream, q);
    HIP_CHECK(hipGetLastError());
    return EGONN_OK;
  }
  hipLaunchKernelGGL(local_heads_kernel, dim3(grid), dim3(LH_WAVES * 64), lds, stream, a);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ top-k (smallest sigma, ascending, ties by row)
// MinkLocGLEvaluator.get_keypoints_idxes (eval/evaluate.py:352-361: torch.topk(sigma, n_k, largest=False) per scan) +
// the gather of the selected keypoints / descriptors, ONE launch: workgroup = scan.  Keys = (monotone sigma bits << 32 |
// row inside the scan) are unique, so the order is total (ties by Z-order row, as the stable radix sort it replaces).
// Radix SELECT, then a sort of the k winners only: 11-bit digits of the 64-bit key from the top, one LDS histogram per
// digit over the rows that still match the prefix, until the tie group is taken whole (two or three passes on real
// saliencies, six at most: the keys are unique) -> a threshold key; the k keys at or below it are compacted into LDS and
// ordered by counting (k <= 512) or by a bitonic network.  (The r01/r02 kernel sorted the whole scan through a 2048-key
// bitonic network, 66 barrier stages per 1920 rows: 49 us at 23 k rows per scan.)
__device__ static inline uint32_t sigma_bits(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // monotone float -> uint
}
constexpr int TK_THREADS = 1024, TK_BINS = 2048, TK_CACHE = 8;
__global__ __launch_bounds__(TK_THREADS) void select_topk_kernel(const float* __restrict__ sigma, const int32_t* __restrict__ boff,
                                                                 int k, int S, const float* __restrict__ kp,
                                                                 const float* __restrict__ desc, int dc,
                                                                 int32_t* __restrict__ sel_rows, int32_t* __restrict__ sel_count,
                                                                 float* __restrict__ out_kp, float* __restrict__ out_desc) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long skeys[];   // [S] winners, S = pow2 >= k; + [k] when ranked
  __shared__ uint32_t s_hist[TK_BINS];
  __shared__ uint32_t s_wave[TK_THREADS / 64];
  __shared__ uint32_t s_pick[3];                         // digit, rows below it, rows in it
  __shared__ uint32_t s_n;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t r0 = boff[b], nb = boff[b + 1] - r0;
  const int kk = min(k, nb);
  // the scan's keys: the first TK_CACHE * 1024 rows stay in registers, longer scans re-read the tail
  uint32_t sb[TK_CACHE];
#pragma unroll
  for (int i = 0; i < TK_CACHE; ++i) {
    const int r = i * TK_THREADS + tid;
    sb[i] = r < nb ? sigma_bits(sigma[r0 + r]) : 0xFFFFFFFFu;
  }
  auto key_of = [&](uint32_t bits, int r) { return ((unsigned long long)bits << 32) | (unsigned)r; };
  unsigned long long T = 0;                              // threshold: the kk smallest keys are the keys <= T
  if (kk > 0) {
    unsigned long long prefix = 0;
    uint32_t need = (uint32_t)kk;
    const int shifts[6] = {53, 42, 31, 20, 9, 0};
#pragma unroll 1
    for (int p = 0; p < 6; ++p) {
      const int sh = shifts[p], bits = p == 5 ? 9 : 11;
      const uint32_t dmask = (1u << bits) - 1;
      for (int i = tid; i < TK_BINS; i += TK_THREADS) s_hist[i] = 0;
      __syncthreads();
      auto count = [&](uint32_t sbits, int r) {
        const unsigned long long key = key_of(sbits, r);
        if (p == 0 || (key >> (sh + bits)) == prefix) atomicAdd(&s_hist[(uint32_t)(key >> sh) & dmask], 1u);
      };
#pragma unroll
      for (int i = 0; i < TK_CACHE; ++i) {
        const int r = i * TK_THREADS + tid;
        if (r < nb) count(sb[i], r);
      }
      for (int r = TK_CACHE * TK_THREADS + tid; r < nb; r += TK_THREADS) count(sigma_bits(sigma[r0 + r]), r);
      __syncthreads();
      // digit that holds the need-th smallest key: exclusive scan of the histogram, two bins per thread
      const uint32_t h0 = s_hist[2 * tid], h1 = s_hist[2 * tid + 1];
      uint32_t inc = h0 + h1;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
      }
      if (lane == 63) s_wave[wave] = inc;
      __syncthreads();
      uint32_t ex = inc - (h0 + h1);
      for (int w = 0; w < wave; ++w) ex += s_wave[w];
      if (ex < need && need <= ex + h0) {
        s_pick[0] = 2 * tid; s_pick[1] = ex; s_pick[2] = h0;
      } else if (ex + h0 < need && need <= ex + h0 + h1) {
        s_pick[0] = 2 * tid + 1; s_pick[1] = ex + h0; s_pick[2] = h1;
      }
      __syncthreads();
      const uint32_t digit = s_pick[0], below = s_pick[1], inbin = s_pick[2];
      prefix = (prefix << bits) | digit;
      need -= below;
      if (inbin == need || sh == 0) {                    // the tie group is taken whole
        T = sh ? ((prefix << sh) | ((1ull << sh) - 1)) : prefix;
        break;
      }
    }
  }
  // ---- the kk winners -> LDS (any order), then ordered
  if (tid == 0) s_n = 0;
  for (int i = tid; i < S; i += TK_THREADS) skeys[i] = ~0ull;
  __syncthreads();
  if (kk > 0) {
    auto take = [&](uint32_t sbits, int r) {
      const unsigned long long key = key_of(sbits, r);
      if (key <= T) skeys[atomicAdd(&s_n, 1u)] = key;
    };
#pragma unroll
    for (int i = 0; i < TK_CACHE; ++i) {
      const int r = i * TK_THREADS + tid;
      if (r < nb) take(sb[i], r);
    }
    for (int r = TK_CACHE * TK_THREADS + tid; r < nb; r += TK_THREADS) take(sigma_bits(sigma[r0 + r]), r);
  }
  __syncthreads();
  if (k <= 512) {                                        // order by counting: every key reads all the others (broadcasts)
    unsigned long long* sorted = skeys + S;
    if (tid < kk) {
      const unsigned long long mine = skeys[tid];
      int rank = 0;
      for (int j = 0; j < kk; ++j) rank += skeys[j] < mine ? 1 : 0;
      sorted[rank] = mine;
    }
    __syncthreads();
    if (tid < kk) skeys[tid] = sorted[tid];
    __syncthreads();
  } else {
    for (int k2 = 2; k2 <= S; k2 <<= 1)
      for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
        for (int e = tid; e < S / 2; e += TK_THREADS) {
          const int i = ((e & ~(j2 - 1)) << 1) | (e & (j2 - 1));
          const int q = i | j2;
          const bool up = (i & k2) == 0;
          const unsigned long long x = skeys[i], y = skeys[q];
          if ((x > y) == up) { skeys[i] = y; skeys[q] = x; }
        }
        __syncthreads();
      }
  }
  // ---- selected rows + gathered keypoints / descriptors (padded with -1 / zeros)
  for (int i = tid; i < k; i += TK_THREADS) sel_rows[(int64_t)b * k + i] = (i < kk) ? r0 + (int32_t)(skeys[i] & 0xFFFFFFFFu) : -1;
  if (tid == 0) sel_count[b] = kk;
  if (out_desc) {
    if ((dc & 3) == 0) {                                 // 16-byte pieces of the descriptor rows
      const int q4 = dc >> 2;
      for (int t = tid; t < k * q4; t += TK_THREADS) {
        const int i = t / q4, c = t - i * q4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < kk) v = *reinterpret_cast<const float4*>(desc + (int64_t)(r0 + (int32_t)(skeys[i] & 0xFFFFFFFFu)) * dc + 4 * c);
        *reinterpret_cast<float4*>(out_desc + ((int64_t)b * k + i) * dc + 4 * c) = v;
      }
    } else {
      for (int64_t t = tid; t < (int64_t)k * dc; t += TK_THREADS) {
        const int i = (int)(t / dc), c = (int)(t - (int64_t)i * dc);
        out_desc[((int64_t)b * k + i) * dc + c] = (i < kk) ? desc[(int64_t)(r0 + (int32_t)(skeys[i] & 0xFFFFFFFFu)) * dc + c] : 0.f;
      }
    }
    for (int t = tid; t < k * 3; t += TK_THREADS) {
      const int i = t / 3, c = t - i * 3;
      out_kp[((int64_t)b * k + i) * 3 + c] = (i < kk) ? kp[(int64_t)(r0 + (int32_t)(skeys[i] & 0xFFFFFFFFu)) * 3 + c] : 0.f;
    }
  }
}
int select_topk(const float* sigma, const int32_t* boff_dev, int B, int k, const float* kp, const float* desc, int dc,
                int32_t* sel_rows, int32_t* sel_count, float* out_kp, float* out_desc, hipStream_t stream) {
  EGONN_REQUIRE(k >= 1 && k <= 8192, EGONN_ERR_INVALID, "select_keypoints: n_k=%d outside [1, 8192]", k);
  int S = 64;
  while (S < k) S <<= 1;
  const size_t lds = (size_t)(S + (k <= 512 ? k : 0)) * sizeof(unsigned long long);
  static AttrOnce attr_done;
  if (attr_done.need()) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&select_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  128 * 1024));
    attr_done.mark(); 
  }
  hipLaunchKernelGGL(select_topk_kernel, dim3(B), dim3(TK_THREADS), lds, stream, sigma, boff_dev, k, S, kp, desc, dc, sel_rows,
                     sel_count, out_kp, out_desc);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn
