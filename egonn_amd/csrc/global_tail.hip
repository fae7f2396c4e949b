// The tail of the global head in ONE launch: the descriptor decoder (Linear 128 -> 192 + ReLU, Linear 192 -> 256) and the partial
// sums of the global pooling over its output.  The three launches it replaces (dense_small_kernel, dense_lds_kernel,
// segment_partial_kernel) write the hidden map and the decoder output to memory and read each back once; here neither leaves the
// workgroup.
//
// Reference call sites: global_descriptor_decoder models/minkgl.py:207-217 ; GeM / MAC / SPoC layers/pooling.py:46-86.
#include "common.h"
#include "kernels.h"
#include "rowmath.h"

namespace egonn {

constexpr int GT_KS0 = GTAIL_CIN / 16, GT_KS1 = GTAIL_MID / 16;       // 16-deep contraction blocks of the two layers
constexpr int GT_NT0 = GTAIL_MID / 16 / 4, GT_NT1 = GTAIL_OUT / 16 / 4;   // 16-column tiles per wave: 3 hidden, 4 output
constexpr int GT_HS = GTAIL_MID + 4, GT_OS = GTAIL_OUT + 4;           // LDS row strides (16-byte aligned, rows on different banks)

// grid (SEG_CHUNKS, B): workgroup (ch, b) owns the rows [r0, r1) that segment_partial_kernel gives block (ch, b) and leaves the same
// partial[b][ch][256].  Per 16-row tile the four waves split the output columns of both layers; a wave reads only its own column
// slice of the packed fragments (dense_pack_frags), 16 bytes per lane straight from L2 — the 295 KB set is not staged.  The hidden
// tile goes through LDS; the output tile is staged in LDS and thread c adds its channel's rows in ascending row order, carrying the
// running value over the tiles of a chunk of more than 16 rows.
// Arithmetic of the launches replaced, so that `partial` is bitwise theirs: per output element acc = 0, t ascending, u = 0..3 on
// v_mfma_f32_16x16x4_f32; hidden = relu(acc + b0) with the operand order of dense_small_body; output = the epilogue expression of
// dense_lds_kernel with its operand order; the loop and the second stage of segment_partial_kernel at c = 256.
// Rows past the end of a chunk repeat its last row (computed, never added): no row outside [r0, r1) is read.
__global__ __launch_bounds__(256, 2) void global_tail_kernel(const float* __restrict__ g5, int64_t ncap, const int32_t* __restrict__ boff,
                                                             const f32x4* __restrict__ wf0, const float* __restrict__ b0,
                                                             const f32x4* __restrict__ wf1, const float* __restrict__ b1, int pow_mode,
                                                             const float* __restrict__ pexp, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float s_hid[16 * GT_HS];
  __shared__ __attribute__((aligned(16))) float s_out[16 * GT_OS];
  const int b = blockIdx.y, ch = blockIdx.x;
  const int32_t s = boff[b], e = boff[b + 1];
  const int64_t len = e - s;
  const int32_t r0 = s + (int32_t)(len * ch / SEG_CHUNKS);
  const int32_t r1 = ncap > 0 ? s + (int32_t)(len * (ch + 1) / SEG_CHUNKS) : r0;      // (no buffer: every chunk is empty)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g4 = lane >> 4;
  const float p = pow_mode == 1 ? pexp[0] : 1.f;           // pow_mode: 0 = sum, 1 = sum of clamp(x)^p (GeM), 2 = max (MAC)
  float run = pow_mode == 2 ? -INFINITY : 0.f;
#pragma unroll 1
  for (int32_t base = r0; base < r1; base += 16) {
    // (the fragment loads do not depend on the tile: behind an opaque zero they stay inside the loop, where a tile's share fits the
    // registers — hoisted out of it, all 84 are live at once and spill)
    int zero = 0;
    asm volatile("" : "+s"(zero));
    const f32x4* const w0p = wf0 + (int64_t)wave * GT_NT0 * GT_KS0 * 64 + lane + zero;
    const f32x4* const w1p = wf1 + (int64_t)wave * GT_NT1 * GT_KS1 * 64 + lane + zero;
    // ---- requests: the tile's rows, the wave's hidden-layer fragments and bias values, the fragments of its first output tile
    const int64_t row = max(min((int64_t)min(base + l15, r1 - 1), ncap - 1), (int64_t)0);
    f32x4 a[GT_KS0], w0[GT_NT0][GT_KS0], w1[2][GT_KS1];
    float bh[GT_NT0];
#pragma unroll
    for (int t = 0; t < GT_KS0; ++t) a[t] = *reinterpret_cast<const f32x4*>(g5 + row * GTAIL_CIN + 16 * t + 4 * g4);
#pragma unroll
    for (int j = 0; j < GT_NT0; ++j) {
#pragma unroll
      for (int t = 0; t < GT_KS0; ++t) w0[j][t] = w0p[(j * GT_KS0 + t) * 64];
      bh[j] = b0[16 * (wave * GT_NT0 + j) + l15];
    }
#pragma unroll
    for (int t = 0; t < GT_KS1; ++t) w1[0][t] = w1p[t * 64];
    __builtin_amdgcn_sched_barrier(0);
    // ---- hidden tile -> LDS: lane (column l15 of the tile, rows 4 g4 .. 4 g4 + 3), as in dense_small_body
#pragma unroll
    for (int j = 0; j < GT_NT0; ++j) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < GT_KS0; ++t) {
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][u], w0[j][t][u], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s_hid[(4 * g4 + r) * GT_HS + 16 * (wave * GT_NT0 + j) + l15] = fmaxf(acc[r] + bh[j], 0.f);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    f32x4 h[GT_KS1];
#pragma unroll
    for (int t = 0; t < GT_KS1; ++t) h[t] = *reinterpret_cast<const f32x4*>(s_hid + l15 * GT_HS + 16 * t + 4 * g4);
    __builtin_amdgcn_sched_barrier(0);
    // ---- output tile -> LDS: lane (row l15, four consecutive columns), as in dense_lds_kernel; the next column tile's fragments
    // are in flight behind the MFMAs of this one
#pragma unroll
    for (int j = 0; j < GT_NT1; ++j) {
      const int c0 = 16 * (wave * GT_NT1 + j) + 4 * g4;
      const f32x4 bo = *reinterpret_cast<const f32x4*>(b1 + c0);
      if (j + 1 < GT_NT1) {
#pragma unroll
        for (int t = 0; t < GT_KS1; ++t) w1[(j + 1) & 1][t] = w1p[((j + 1) * GT_KS1 + t) * 64];
      }
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < GT_KS1; ++t) {
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[j & 1][t][u], h[t][u], acc, 0, 0, 0);
      }
      f32x4 v = acc + bo;
      v = v * 1.f + 0.f;                                     // scale / shift of a layer without BatchNorm (-0 becomes +0)
      *reinterpret_cast<f32x4*>(s_out + l15 * GT_OS + c0) = v;
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    // ---- thread c adds channel c of the tile's live rows.  (The next tile writes s_hid before its first barrier — every read of it
    // is behind the barrier above — and s_out after it, when every thread has left this loop.)
    const int nrows = min(16, r1 - base);
    for (int r = 0; r < nrows; ++r) {
      float v = s_out[r * GT_OS + tid];
      if (pow_mode == 1) v = powf(fmaxf(v, 1e-6f), p);
      run = pow_mode == 2 ? fmaxf(run, v) : run + v;
    }
  }
  float sum = pow_mode == 2 ? -INFINITY : 0.f;               // the second stage of segment_partial_kernel at c = 256: one term
  sum = pow_mode == 2 ? fmaxf(sum, run) : sum + run;
  partial[((int64_t)b * SEG_CHUNKS + ch) * GTAIL_OUT + tid] = sum;
}

int global_tail_fused(const float* g5, int64_t ncap, const int32_t* boff, int B, const float* wf0, const float* b0, const float* wf1,
                      const float* b1, int pow_mode, const float* p, float* partial, hipStream_t stream) {
  EGONN_REQUIRE(g5 && boff && wf0 && b0 && wf1 && b1 && partial && B >= 1 && ncap >= 0 && pow_mode >= 0 && pow_mode <= 2 &&
                    (pow_mode != 1 || p),
                EGONN_ERR_INVALID, "global tail: bad arguments");
  hipLaunchKernelGGL(global_tail_kernel, dim3(SEG_CHUNKS, B), dim3(256), 0, stream, g5, ncap, boff, reinterpret_cast<const f32x4*>(wf0),
                     b0, reinterpret_cast<const f32x4*>(wf1), b1, pow_mode, p, partial);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn
