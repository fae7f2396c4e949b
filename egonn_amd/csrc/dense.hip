// The 1x1 convolutions / nn.Linear layers of the forward on exact-f32 MFMA: five kernels for one product, the packer of their
// LDS fragment order, and the host side — a layer is a DenseCall, dense_route alone picks its kernel, dense_forward launches it.
//
// Reference call sites: MinkowskiConvolution(k=1) models/minkgl.py:43,124 ; MinkowskiLinear models/minkgl.py:167-217.
#include <algorithm>
#include <type_traits>

#include "../../include/egonn_hip.h"
#include "common.h"
#include "kernels.h"
#include "rowmath.h"

namespace egonn {

// ------------------------------------------------------------------ dense GEMM + epilogue
// Workgroup = 64 rows x 64 output columns (grid.y walks the column groups), wave = 16 rows x 64 columns as two
// passes of two 16-wide v_mfma_f32_16x16x4_f32 column tiles.  The wave's A fragment (16 rows x CIN) is loaded
// once into registers; all B loads of a pass are issued before its MFMA chains (CIN is a template parameter so
// the loops unroll and the loads batch).  The contraction index inside a 16-wide k-block is permuted (lane
// group g owns ci = 16t + 4g .. 4g+3) so that A and (out,in)-layout B come in as one float4 per lane.
// IN_BF16: the input rows are bf16 (configs[2] feature maps; widened exactly to fp32 in registers — the weights and the
// arithmetic stay fp32); io bit 0: residual is bf16, bit 1: out is bf16.
template <int W_OUT_IN, int CIN, bool IN_BF16>
__global__ __launch_bounds__(256) void dense_kernel(const void* __restrict__ in_v, int64_t n,
                                                    const float* __restrict__ W, int cout,
                                                    const float* __restrict__ bias, const float* __restrict__ scale,
                                                    const float* __restrict__ shift, int act,
                                                    const void* __restrict__ residual_v, void* __restrict__ out_v, int io,
                                                    const int32_t* __restrict__ n_dev) {
  if (n_dev) n = min((int64_t)*n_dev, n);               // reserved plans: the grid is sized for the capacity
  const float* in = reinterpret_cast<const float*>(in_v);
  const float* residual = reinterpret_cast<const float*>(residual_v);
  float* out = reinterpret_cast<float*>(out_v);
  constexpr int KS = CIN / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, g4 = lane >> 4;
  const int64_t row_base = ((int64_t)blockIdx.x * 4 + wave) * 16;
  if (row_base >= n) return;
  const int64_t row = row_base + l15;
  float4 a[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) {
    a[t] = make_float4(0, 0, 0, 0);
    if (row < n) {
      if constexpr (IN_BF16) {
        const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(in_v) + row * CIN + 16 * t + 4 * g4);
        a[t] = make_float4(bf2f(h.x & 0xFFFFu), bf2f(h.x >> 16), bf2f(h.y & 0xFFFFu), bf2f(h.y >> 16));
      } else {
        a[t] = *reinterpret_cast<const float4*>(in + row * CIN + 16 * t + 4 * g4);
      }
    }
  }
  const int ncol0 = blockIdx.y * 64;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const int n0 = ncol0 + pass * 32;
    if (n0 >= cout) break;
    float4 b[2][KS];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int col = n0 + nt * 16 + l15;
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        float4 v = make_float4(0, 0, 0, 0);
        if (col < cout) {
          if (W_OUT_IN) {
            v = *reinterpret_cast<const float4*>(W + (int64_t)col * CIN + 16 * t + 4 * g4);
          } else {
            const float* wp = W + (int64_t)(16 * t + 4 * g4) * cout + col;
            v.x = wp[0];
            v.y = wp[cout];
            v.z = wp[2 * (int64_t)cout];
            v.w = wp[3 * (int64_t)cout];
          }
        }
        b[nt][t] = v;
      }
    }
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int t = 0; t < KS; ++t) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, b[nt][t].x, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, b[nt][t].y, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, b[nt][t].z, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, b[nt][t].w, acc[nt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int col = n0 + nt * 16 + l15;
      if (col < cout) {
        const float bi = bias ? bias[col] : 0.f;
        const float sc = scale ? scale[col] : 1.f, sh = scale ? shift[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t orow = row_base + 4 * g4 + r;
          if (orow < n) {
            float v = acc[nt][r] + bi;
            if (scale) v = v * sc + sh;
            v = apply_act(v, act);
            if (residual_v)
              v += (io & 1) ? bf2f(reinterpret_cast<const uint16_t*>(residual_v)[orow * cout + col]) : residual[orow * cout + col];
            if (io & 2) reinterpret_cast<uint16_t*>(out_v)[orow * cout + col] = (uint16_t)f2bf_rn(v);
            else out[orow * cout + col] = v;
          }
        }
      }
    }
  }
}

// dense_small_kernel: the same tile arithmetic for launches too small to hide latency (n < 8192 rows) — see its first comment.
template <int W_OUT_IN, int CIN, bool IN_BF16>
__device__ static inline __attribute__((always_inline)) void dense_small_body(const void* __restrict__ in_v, int64_t n,
                                               const float* __restrict__ W, int cout,
                                               const float* __restrict__ bias, const float* __restrict__ scale,
                                               const float* __restrict__ shift, int act,
                                               const void* __restrict__ residual_v, void* __restrict__ out_v, int io,
                                               const int32_t* __restrict__ n_dev, const int block_x, const int block_y) {
  // ONE memory round trip per wave: the live row count, the 16 input rows, the weights of all four 16-column tiles,
  // the epilogue vectors and the residual values are all requested before anything is waited for (the first version
  // walked a chain of five dependent round trips — count, rows, weights of pass 0, its epilogue vectors, weights of
  // pass 1 ... — and took 12-14 us on launches of a dozen workgroups, eight times per step: profiles/r02x_timeline.txt).
  // `n` is the capacity of the buffers, so rows between the live count and `n` may be read (never stored).
  const int64_t ncap = n;
  const int32_t* nd = n_dev ? n_dev : reinterpret_cast<const int32_t*>(W);      // every load below is unconditional:
  const int32_t nlive_raw = *nd;                                                // indices are clamped into the buffers and
  const int32_t nlive32 = n_dev ? nlive_raw : 0x7FFFFFFF;                       // null pointers replaced by W, so the code is
  const float* in = reinterpret_cast<const float*>(in_v);                       // one straight line of requests followed by
  float* out = reinterpret_cast<float*>(out_v);                                 // one wait (guarded loads compiled into a
  constexpr int KS = CIN / 16;                                                  // branch and a partial wait per load)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, g4 = lane >> 4;
  const int64_t row_base = ((int64_t)block_x * 4 + wave) * 16;
  if (row_base >= ncap) return;
  const int64_t row = min(row_base + l15, ncap - 1);
  float4 a[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) {
    if constexpr (IN_BF16) {
      const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(in_v) + row * CIN + 16 * t + 4 * g4);
      a[t] = make_float4(bf2f(h.x & 0xFFFFu), bf2f(h.x >> 16), bf2f(h.y & 0xFFFFu), bf2f(h.y >> 16));
    } else {
      a[t] = *reinterpret_cast<const float4*>(in + row * CIN + 16 * t + 4 * g4);
    }
  }
  const int ncol0 = block_y * 64;
  float4 b[4][KS];
  float bi[4], sc[4], sh[4];
  const float* bias_p = bias ? bias : W;
  const float* scale_p = scale ? scale : W;
  const float* shift_p = scale ? shift : W;
  // W_OUT_IN = 2: W is the kernel in fragment order (dense_pack_frags; cout a multiple of 16) — the operand of a column tile is
  // CIN / 16 16-byte loads per lane instead of CIN / 4 strided dword loads (W_OUT_IN = 0)
  auto load_b = [&](int nt) {
    const int col = min(ncol0 + nt * 16 + l15, cout - 1);
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      float4 v;
      if (W_OUT_IN == 2) {
        v = *reinterpret_cast<const float4*>(W + ((int64_t)((col >> 4) * KS + t) * 64 + lane) * 4);
      } else if (W_OUT_IN == 1) {
        v = *reinterpret_cast<const float4*>(W + (int64_t)col * CIN + 16 * t + 4 * g4);
      } else {      // (32-bit unsigned offsets from one scalar base: one address register per load instead of two)
        const uint32_t uc = (uint32_t)cout, o = (uint32_t)(16 * t + 4 * g4) * uc + (uint32_t)col;
        v.x = W[o];
        v.y = W[o + uc];
        v.z = W[o + 2u * uc];
        v.w = W[o + 3u * uc];
      }
      b[nt][t] = v;
    }
  };
  // NUP column tiles' operands are requested up front: all four, except with 128 fp32 input channels and a raw (cin, cout)
  // kernel — 128 strided dword loads, whose results and addresses beside the rows do not fit the 256 registers of two waves per
  // SIMD.  There the operand of the fourth tile is requested after the first tile's MFMAs, into its registers, and lands behind
  // the MFMAs of the second and third.  Same MFMA order per element.
  constexpr int NUP = (CIN >= 128 && !IN_BF16 && W_OUT_IN == 0) ? 3 : 4;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int col = min(ncol0 + nt * 16 + l15, cout - 1);
    bi[nt] = bias_p[col];
    sc[nt] = scale_p[col];
    sh[nt] = shift_p[col];
    if (nt < NUP) load_b(nt);
  }
  float res[4][4];
  {
    const bool has_res = residual_v != nullptr;
    const void* rp = has_res ? residual_v : static_cast<const void*>(W);
    int64_t ridx[4][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int col = min(ncol0 + nt * 16 + l15, cout - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t orow = min(row_base + 4 * g4 + r, ncap - 1);
        ridx[nt][r] = has_res ? orow * cout + col : 0;
      }
    }
    if (io & 1) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) res[nt][r] = bf2f(reinterpret_cast<const uint16_t*>(rp)[ridx[nt][r]]);
    } else {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) res[nt][r] = reinterpret_cast<const float*>(rp)[ridx[nt][r]];
    }
  }
  if (!bias) bi[0] = bi[1] = bi[2] = bi[3] = 0.f;
  n = min((int64_t)nlive32, ncap);
  if (row_base >= n) return;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int col = ncol0 + nt * 16 + l15;
    if (ncol0 + nt * 16 >= cout) break;
    if constexpr (NUP < 4) {
      if (nt >= 1 && nt + NUP - 1 < 4) load_b(nt + NUP - 1);
      __builtin_amdgcn_sched_barrier(0);      // (the request stays between the first and the second tile's MFMAs)
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, b[nt][t].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, b[nt][t].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, b[nt][t].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, b[nt][t].w, acc, 0, 0, 0);
    }
    if (col < cout) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t orow = row_base + 4 * g4 + r;
        if (orow < n) {
          float v = acc[r] + bi[nt];
          if (scale) v = v * sc[nt] + sh[nt];
          v = apply_act(v, act);
          if (residual_v) v += res[nt][r];
          if (io & 2) reinterpret_cast<uint16_t*>(out_v)[orow * cout + col] = (uint16_t)f2bf_rn(v);
          else out[orow * cout + col] = v;
        }
      }
    }
  }
}

template <int W_OUT_IN, int CIN, bool IN_BF16>
__global__ __launch_bounds__(256) void dense_small_kernel(const void* __restrict__ in_v, int64_t n,
                                                    const float* __restrict__ W, int cout,
                                                    const float* __restrict__ bias, const float* __restrict__ scale,
                                                    const float* __restrict__ shift, int act,
                                                    const void* __restrict__ residual_v, void* __restrict__ out_v, int io,
                                                    const int32_t* __restrict__ n_dev) {
  dense_small_body<W_OUT_IN, CIN, IN_BF16>(in_v, n, W, cout, bias, scale, shift, act, residual_v, out_v, io, n_dev, (int)blockIdx.x,
                                           (int)blockIdx.y);
}
// Up to three INDEPENDENT small products of one shape in one launch (the three lateral 1x1 convolutions of MinkHead,
// models/minkgl.py:46-60: they depend on the trunk only, not on each other): block ranges of one grid, the body of the kernel above.
struct DenseGroup3 {
  const void* in[3];
  const float* W[3];
  void* out[3];
  const int32_t* n_dev[3];
  int64_t n[3];
  int bx0[4];                // first block of every problem along grid.x
};
template <int W_OUT_IN, int CIN, bool IN_BF16>
__global__ __launch_bounds__(256) void dense_small3_kernel(const DenseGroup3 g, int cout, int io) {
  const int b = (int)blockIdx.x;
  const int q = b >= g.bx0[2] ? 2 : (b >= g.bx0[1] ? 1 : 0);
  dense_small_body<W_OUT_IN, CIN, IN_BF16>(g.in[q], g.n[q], g.W[q], cout, nullptr, nullptr, nullptr, ACT_NONE, nullptr, g.out[q], io,
                                           g.n_dev[q], b - g.bx0[q], (int)blockIdx.y);
}


// The same product with the weights staged ONCE per workgroup into LDS as MFMA fragments
//   frag[(nt * CIN/16 + t) * 64 + lane] = W(col = 16 nt + (lane & 15), ci = 16 t + 4 (lane >> 4) .. +3)
// (whatever the caller's layout), workgroups persistent over the row tiles, operands swapped (D^T = W^T A^T) so that lane
// (row, g) owns four consecutive output columns: the epilogue is one 16-byte load / store per 16 columns.  The kernel
// above re-fetches its 32-64 KB of weights per 16-row tile (dword loads in the (in, out) layout) and stores single
// floats; this one runs the 1x1 convolutions of the heads 2x faster.  Same accumulation order => same results.
// Used when the fragments fit (Cin * Cout * 4 <= 96 KB) and Cout is a multiple of 16.
template <int W_OUT_IN, int CIN, bool IN_BF16>
__global__ __launch_bounds__(256) void dense_lds_kernel(const void* __restrict__ in_v, int64_t n,
                                                        const float* __restrict__ W, int cout,
                                                        const float* __restrict__ bias, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, int act,
                                                        const void* __restrict__ residual_v, void* __restrict__ out_v, int io,
                                                        const int32_t* __restrict__ n_dev, int colblk,
                                                        const float* __restrict__ gate, const int32_t* __restrict__ boff, int B) {
  extern __shared__ __attribute__((aligned(16))) f32x4 dl_frags[];
  if (n_dev) n = min((int64_t)*n_dev, n);
  constexpr int KS = CIN / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g4 = lane >> 4;
  // grid.y splits the output columns into blocks of `colblk` (a multiple of 16) when all the fragments do not fit in LDS
  const int cb0 = blockIdx.y * colblk;
  const int NT = min(colblk, cout - cb0) >> 4, ncl = NT * 16;
  // eight fragments per thread in flight (one at a time made the staging a chain of up to 96 dependent round trips:
  // 24 us for the 96 KB block of the 192 -> 256 layer)
  auto frag_of = [&](int i) -> f32x4 {
    const int ln = i & 63, ft = i >> 6;
    const int nt = ft / KS, t = ft - nt * KS;
    const int col = cb0 + 16 * nt + (ln & 15), k0 = 16 * t + 4 * (ln >> 4);
    if (W_OUT_IN) return *reinterpret_cast<const f32x4*>(W + (int64_t)col * CIN + k0);
    const float* wp = W + (int64_t)k0 * cout + col;
    return (f32x4){wp[0], wp[cout], wp[2 * (int64_t)cout], wp[3 * (int64_t)cout]};
  };
  const int nfrag = NT * KS * 64;
  int i0 = tid;
  for (; i0 + 7 * 256 < nfrag; i0 += 8 * 256) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = frag_of(i0 + u * 256);
#pragma unroll
    for (int u = 0; u < 8; ++u) dl_frags[i0 + u * 256] = v[u];
  }
  for (; i0 < nfrag; i0 += 256) dl_frags[i0] = frag_of(i0);
  __syncthreads();
  // bias / folded-BN vectors of the epilogue -> LDS (behind the fragments): they were three dependent L1 round trips per
  // 16 output columns of every tile
  float* const s_vec = reinterpret_cast<float*>(dl_frags + (int64_t)NT * KS * 64);      // [3][cout]: bias, scale, shift
  for (int i = tid; i < ncl; i += 256) {
    s_vec[i] = bias ? bias[cb0 + i] : 0.f;
    s_vec[ncl + i] = scale ? scale[cb0 + i] : 1.f;
    s_vec[2 * ncl + i] = scale ? shift[cb0 + i] : 0.f;
  }
  __syncthreads();
  const int64_t ntiles = (n + 15) >> 4;
  const int64_t tstep = (int64_t)gridDim.x * 4;
  auto load_rows = [&](int64_t tile, f32x4 (&a)[KS]) {      // the 16 input rows of a tile (zeros past the end)
    const int64_t row = tile * 16 + l15;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      a[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (tile < ntiles && row < n) {
        if constexpr (IN_BF16) {
          const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(in_v) + row * CIN + 16 * t + 4 * g4);
          a[t] = (f32x4){bf2f(h.x & 0xFFFFu), bf2f(h.x >> 16), bf2f(h.y & 0xFFFFu), bf2f(h.y >> 16)};
        } else {
          a[t] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(in_v) + row * CIN + 16 * t + 4 * g4);
        }
      }
    }
  };
  f32x4 a[KS], an[KS];
  int64_t tile = (int64_t)blockIdx.x * 4 + wave;
  load_rows(tile, a);
  for (; tile < ntiles; tile += tstep) {
    const int64_t row = tile * 16 + l15;
    const bool ok = row < n;
    load_rows(tile + tstep, an);                             // next tile's rows in flight while this one is computed
    // gate != null: the ECA tail of a block with a 1x1 downsample branch (layers/eca_block.py:66-73) fused into this launch —
    // out = relu(residual * gate[sample of the row] + this layer's output): the downsample output never goes to memory
    const int64_t gbase = (gate && ok) ? (int64_t)sample_of_row(boff, B, (int32_t)row) * cout : 0;
    for (int nt = 0; nt < NT; ++nt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const f32x4* fr = dl_frags + (int64_t)nt * KS * 64 + lane;
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        const f32x4 wf = fr[t * 64];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[u], a[t][u], acc, 0, 0, 0);
      }
      if (ok) {
        const int cl = 16 * nt + 4 * g4, c0 = cb0 + cl;
        f32x4 v = acc + *reinterpret_cast<const f32x4*>(s_vec + cl);
        v = v * *reinterpret_cast<const f32x4*>(s_vec + ncl + cl) + *reinterpret_cast<const f32x4*>(s_vec + 2 * ncl + cl);
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = apply_act(v[u], act);
        if (residual_v) {
          f32x4 r;
          if (io & 1) {
            const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(residual_v) + row * cout + c0);
            r = (f32x4){bf2f(h.x & 0xFFFFu), bf2f(h.x >> 16), bf2f(h.y & 0xFFFFu), bf2f(h.y >> 16)};
          } else {
            r = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(residual_v) + row * cout + c0);
          }
          if (gate) {
            const f32x4 gq = *reinterpret_cast<const f32x4*>(gate + gbase + c0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              // (bf16 maps: the downsample output was a bf16 map between the two launches this replaces; same rounding here)
              const float d = (io & 2) ? bf2f(f2bf_rn(v[u])) : v[u];
              v[u] = fmaxf(r[u] * gq[u] + d, 0.f);           // the expression of eca_apply_kernel
            }
          } else {
            v += r;
          }
        }
        if (io & 2) {
          *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out_v) + row * cout + c0) =
              make_uint2(f2bf_rn(v[0]) | (f2bf_rn(v[1]) << 16), f2bf_rn(v[2]) | (f2bf_rn(v[3]) << 16));
        } else {
          *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out_v) + row * cout + c0) = v;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < KS; ++t) a[t] = an[t];
  }
}

// Float j of a 1x1 kernel's packed fragment buffer (the LDS image of the two kernels around this comment, whole kernel, cb0 = 0):
//   packed[((nt * cin/16 + t) * 64 + lane) * 4 + u] = W(ci = 16 t + 4 (lane >> 4) + u, col = 16 nt + (lane & 15))
// -> its index in the caller's weights.  One function behind the device packer, the host packer and the on-the-fly staging.
__host__ __device__ static inline int64_t dense_frag_src(int64_t j, int w_out_in, int cin, int cout) {
  const int u = (int)(j & 3), ln = (int)((j >> 2) & 63), ft = (int)(j >> 8), ks = cin / 16;
  const int nt = ft / ks, t = ft - nt * ks;
  const int ci = 16 * t + 4 * (ln >> 4) + u, col = 16 * nt + (ln & 15);
  return w_out_in ? (int64_t)col * cin + ci : (int64_t)ci * cout + col;
}
__global__ void dense_pack_kernel(const float* __restrict__ W, int w_out_in, int cin, int cout, float* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < (int64_t)cin * cout) out[j] = W[dense_frag_src(j, w_out_in, cin, cout)];
}
int dense_pack_frags(const float* W, int w_out_in, int cin, int cout, float* out, hipStream_t stream) {
  EGONN_REQUIRE(W && out && cin >= 16 && cin % 16 == 0 && cout >= 16 && cout % 16 == 0, EGONN_ERR_INVALID,
                "dense pack: %d->%d (multiples of 16 expected)", cin, cout);
  hipLaunchKernelGGL(dense_pack_kernel, dim3((unsigned)cdiv((int64_t)cin * cout, 256)), dim3(256), 0, stream, W, w_out_in ? 1 : 0, cin,
                     cout, out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// Streaming form of dense_lds_kernel: ONE 16-row tile per wave, the grid sized from the capacity alone, and every request of the
// tile — the staged weights (packed at egonn_model_finalize: coalesced 16-byte loads; else gathered from the caller's layout), the
// epilogue vectors, the scan offsets, the input rows and the residual rows of all COUT/16 column tiles — issued before the first
// wait.  The scan of a row is searched in an LDS copy of boff, and the gate rows are requested before the first MFMA.  dense_lds_kernel
// keeps 2 waves per SIMD with 2 KB each in flight and walks a chain of dependent round trips per tile (rows -> search in global
// memory -> residual -> gate -> store); here a CU holds 16 waves with 6-12 KB each in flight.  Same MFMA sequence per tile, same
// epilogue expression => bitwise the results of dense_lds_kernel.  Rows between the live count and the capacity are neither read
// nor written.
// ACT_ANY = false: act is ACT_NONE or ACT_RELU (every 1x1 convolution of the forward) — the unrolled epilogue then carries no
// COUT/4 copies of tanhf / log1pf / expf.
template <int CIN, int COUT, bool IN_BF16, bool ACT_ANY>
__global__ __launch_bounds__(256, 4) void dense_stream_kernel(const void* __restrict__ in_v, int64_t n, const float* __restrict__ W,
                                                           int w_out_in, const float* __restrict__ wfrag,
                                                           const float* __restrict__ bias, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, int act,
                                                           const void* __restrict__ residual_v, void* __restrict__ out_v, int io,
                                                           const int32_t* __restrict__ n_dev, const float* __restrict__ gate,
                                                           const int32_t* __restrict__ boff, int B) {
  extern __shared__ __attribute__((aligned(16))) f32x4 ds_frags[];
  constexpr int KS = CIN / 16, NT = COUT / 16, NFRAG = NT * KS * 64, PER = NFRAG / 256;
  static_assert(NFRAG % 256 == 0, "whole fragments per thread");
  float* const s_vec = reinterpret_cast<float*>(ds_frags + NFRAG);           // [3][COUT]: bias, scale, shift
  int32_t* const s_boff = reinterpret_cast<int32_t*>(s_vec + 3 * COUT);      // [B + 1]
  if (n_dev) n = min((int64_t)*n_dev, n);
  if (!gate) B = 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g4 = lane >> 4;
  // Every load below is unconditional — null pointers are replaced by W (cin * cout floats: every dummy index stays inside it) and
  // rows past the live count by the last live row — so that the requests are one straight line followed by one wait (guarded
  // loads compiled into a branch, a wait and, under the register bound, a spill per load: see dense_small_body).
  // ---- requests: weights (without a packed copy the same bytes of W, overwritten below), vectors, scan offsets
  f32x4 st[PER];
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(wfrag ? wfrag : W);
#pragma unroll
    for (int u = 0; u < PER; ++u) st[u] = src[tid + u * 256];
  }
  const int vi = min(tid, COUT - 1);
  float vb = (bias ? bias : W)[vi], vs = (scale ? scale : W)[vi], vh = (scale ? shift : W)[vi];
  const int32_t vo = (gate ? boff : reinterpret_cast<const int32_t*>(W))[gate ? min(tid, B) : 0];
  // ---- requests: this wave's tile (raw bits; bf16 rows are widened after the barrier)
  const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * 16 + l15;
  const bool ok = row < n;
  const int64_t rowc = min(row, max(n, (int64_t)1) - 1);
  f32x4 a[KS], r[NT];
#pragma unroll
  for (int t = 0; t < KS; ++t) {
    if constexpr (IN_BF16) {
      const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(in_v) + rowc * CIN + 16 * t + 4 * g4);
      a[t] = (f32x4){__uint_as_float(h.x), __uint_as_float(h.y), 0.f, 0.f};
    } else {
      a[t] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(in_v) + rowc * CIN + 16 * t + 4 * g4);
    }
  }
  {
    const void* rp = residual_v ? residual_v : static_cast<const void*>(W);
    const int64_t r0 = (residual_v ? rowc * COUT : 0) + 4 * g4;
    if (io & 1) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(rp) + r0 + 16 * nt);
        r[nt] = (f32x4){__uint_as_float(h.x), __uint_as_float(h.y), 0.f, 0.f};
      }
    } else {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) r[nt] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(rp) + r0 + 16 * nt);
    }
  }
  // ---- LDS image
#pragma unroll
  for (int u = 0; u < PER; ++u) ds_frags[tid + u * 256] = st[u];
  if (!wfrag) {      // no packed copy (stand-alone callers): gathered from the caller's layout, one fragment per thread at a time
#pragma unroll 1
    for (int i = tid; i < NFRAG; i += 256) {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = W[dense_frag_src((int64_t)i * 4 + k, w_out_in, CIN, COUT)];
      ds_frags[i] = v;
    }
  }
  if (tid < COUT) {
    s_vec[tid] = bias ? vb : 0.f;
    s_vec[COUT + tid] = scale ? vs : 1.f;
    s_vec[2 * COUT + tid] = scale ? vh : 0.f;
  }
  if (tid <= B) s_boff[tid] = vo;
  for (int i = tid + 256; i <= B; i += 256) s_boff[i] = boff[i];     // (batches of 256 scans and more; B = 0 without a gate)
  __syncthreads();
  if (((int64_t)blockIdx.x * 4 + wave) * 16 >= n) return;
  // ---- scan of the row (last b with boff[b] <= row) from the LDS copy, then the gate rows: L2 hits, in flight under the MFMAs' operands
  f32x4 gq[NT];
  {
    int lo = 0, hi = gate ? B : 0;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_boff[mid] <= (int32_t)row) lo = mid; else hi = mid;
    }
    const float* gp = (gate ? gate : W) + ((gate && ok) ? (int64_t)lo * COUT : 0) + 4 * g4;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) gq[nt] = *reinterpret_cast<const f32x4*>(gp + 16 * nt);
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (IN_BF16) {
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const uint32_t hx = __float_as_uint(a[t][0]), hy = __float_as_uint(a[t][1]);
      a[t] = (f32x4){bf2f(hx & 0xFFFFu), bf2f(hx >> 16), bf2f(hy & 0xFFFFu), bf2f(hy >> 16)};
    }
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const f32x4* fr = ds_frags + nt * KS * 64 + lane;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const f32x4 wf = fr[t * 64];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[u], a[t][u], acc, 0, 0, 0);
    }
    if (ok) {
      const int c0 = 16 * nt + 4 * g4;
      f32x4 v = acc + *reinterpret_cast<const f32x4*>(s_vec + c0);
      v = v * *reinterpret_cast<const f32x4*>(s_vec + COUT + c0) + *reinterpret_cast<const f32x4*>(s_vec + 2 * COUT + c0);
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ACT_ANY ? apply_act(v[u], act) : (act == ACT_RELU ? fmaxf(v[u], 0.f) : v[u]);
      if (residual_v) {
        f32x4 rr = r[nt];
        if (io & 1) {
          const uint32_t hx = __float_as_uint(rr[0]), hy = __float_as_uint(rr[1]);
          rr = (f32x4){bf2f(hx & 0xFFFFu), bf2f(hx >> 16), bf2f(hy & 0xFFFFu), bf2f(hy >> 16)};
        }
        if (gate) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float d = (io & 2) ? bf2f(f2bf_rn(v[u])) : v[u];     // (see dense_lds_kernel)
            v[u] = fmaxf(rr[u] * gq[nt][u] + d, 0.f);
          }
        } else {
          v += rr;
        }
      }
      if (io & 2) {
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out_v) + row * COUT + c0) =
            make_uint2(f2bf_rn(v[0]) | (f2bf_rn(v[1]) << 16), f2bf_rn(v[2]) | (f2bf_rn(v[3]) << 16));
      } else {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out_v) + row * COUT + c0) = v;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

__global__ void dense_any_kernel(const float* __restrict__ in, int64_t total, int cin, const float* __restrict__ W,
                                 int w_out_in, int cout, const float* __restrict__ bias, int act, float* __restrict__ out,
                                 const int32_t* __restrict__ n_dev) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n_dev) total = min((int64_t)*n_dev * cout, total);
  if (i >= total) return;
  const int64_t r = i / cout;
  const int co = (int)(i - r * cout);
  float s = bias ? bias[co] : 0.f;
  for (int ci = 0; ci < cin; ++ci) s = fmaf(in[r * cin + ci], w_out_in ? W[(int64_t)co * cin + ci] : W[(int64_t)ci * cout + co], s);
  out[i] = apply_act(s, act);
}

// ------------------------------------------------------------------ host side: the route of a layer, then its launch
// Every threshold of the rule, once.  (Measured, batch 16 / 64: from 8192 rows on staged weights win over dense_small_kernel; from
// 2048 on column blocks win over the 64-column kernel, which re-reads its 48 KB weight slice per wave: 17 / 56 -> 18 / 41 us.)
constexpr int64_t DENSE_STAGED_ROWS = 8192;            // rows from which the weights are staged in LDS (streaming or persistent)
constexpr int64_t DENSE_STAGED_ROWS_SPLIT = 2048;      // the same for a weight set split into column blocks
constexpr size_t DENSE_STREAM_MAX_BYTES = 32 * 1024;   // streaming form: weight bytes with which four workgroups share a CU
constexpr size_t DENSE_LDS_BLOCK_BYTES = 96 * 1024;    // persistent kernel: weight bytes per column block (grid.y walks the blocks)
constexpr size_t DENSE_LDS_TWO_WG_BYTES = 72 * 1024;   // column blocks up to this size leave a CU room for two workgroups:
constexpr int DENSE_LDS_WGS[2] = {512, 256};           // persistent workgroups with such blocks, with larger ones
constexpr int DENSE_SMALL_MAX_CIN = 128;               // dense_small_kernel keeps the B operand of four column tiles in registers

// run-time value -> compile-time constant: f(std::integral_constant<int, V>{}) for the V of the list that equals v; false: none does
template <int... V, class F>
static bool pick(int v, F&& f) { return ((v == V && (f(std::integral_constant<int, V>{}), true)) || ...); }
// the channel plans with an MFMA instantiation
template <class F>
static bool pick_cin(int cin, F&& f) { return pick<32, 64, 96, 128, 192, 256>(cin, f); }
// f(CIN, W_OUT_IN, IN_BF16) with the template arguments of dense_kernel / dense_small_kernel / dense_lds_kernel for a call
template <class F>
static void dense_dispatch(const DenseCall& c, F&& f) {
  pick_cin(c.cin, [&](auto CI) { pick<0, 1>(c.w_out_in != 0, [&](auto WOI) { pick<0, 1>(c.in_bf16 != 0, [&](auto INB) {
    f(CI, WOI, std::bool_constant<INB != 0>{}); }); }); });
}
// plans of the streaming form: whole fragments per thread, all of a tile's requests in registers, four workgroups to a CU
constexpr bool dense_stream_plan(int cin, int cout) {
  return (cin == 32 || cin == 64 || cin == 128) && (cout == 64 || cout == 128) && (size_t)cin * cout * sizeof(float) <= DENSE_STREAM_MAX_BYTES;
}

DenseLaunch dense_launch(int64_t n, int cin, int cout, int form, int gate_scans) {
  DenseLaunch l;
  if (n == 0) return l;
  const size_t wbytes = (size_t)cin * cout * sizeof(float);
  const unsigned wave_tiles = (unsigned)cdiv(cdiv(n, 16), 4);        // workgroups of four waves with one 16-row tile per wave
  const bool stream_shape = n >= DENSE_STAGED_ROWS && dense_stream_plan(cin, cout);
  // weight sets above one block (the 192 -> 256 layer of the global decoder) are split over grid.y into column blocks that fit
  const int ysplit = (int)cdiv((int64_t)wbytes, DENSE_LDS_BLOCK_BYTES);
  if (form == 1 && !stream_shape) {
    l.route = DENSE_INVALID;
  } else if (form == 1 || (form < 0 && !switches().no_dense_stream && stream_shape)) {
    l = {DENSE_STREAM, wave_tiles, 1, wbytes + 3 * cout * sizeof(float) + ((size_t)gate_scans + 1) * sizeof(int32_t)};   // + vectors, scan offsets
  } else if (!pick_cin(cin, [](auto) {})) {
    l = {DENSE_PLAIN, (unsigned)cdiv(n * cout, 256), 1};     // (the 3- and 1-channel gradients of the keypoint / sigma regressors)
  } else if (cout % 16 == 0 && n >= (ysplit == 1 ? DENSE_STAGED_ROWS : DENSE_STAGED_ROWS_SPLIT)) {
    const int colblk = (int)(cdiv(cdiv(cout, ysplit), 16) * 16);
    const size_t blk_bytes = (size_t)cin * colblk * sizeof(float);
    const unsigned ny = (unsigned)cdiv(cout, colblk);
    l = {DENSE_LDS, std::min(wave_tiles, DENSE_LDS_WGS[blk_bytes > DENSE_LDS_TWO_WG_BYTES] / ny), ny, blk_bytes + 3 * colblk * sizeof(float), colblk};
  } else {
    l = {n < DENSE_STAGED_ROWS && cin <= DENSE_SMALL_MAX_CIN ? DENSE_SMALL : DENSE_TILE, (unsigned)cdiv(n, 64), (unsigned)cdiv(cout, 64)};
  }
  return l;
}
DenseRoute dense_route(int64_t n, int cin, int cout, int form) { return dense_launch(n, cin, cout, form, 0).route; }
bool dense_gate_fusable(int64_t n, int cin, int cout) {
  const DenseLaunch l = dense_launch(n, cin, cout, 0, 0);
  return l.route == DENSE_LDS && l.gy == 1;
}
// The launch of a layer with rows, or dense_forward's error for a gate (B scans; 0: it came without residual or scan offsets) or a
// form that the shape does not have
static int dense_plan(int64_t n, int cin, int cout, int form, bool gate, int B, DenseLaunch* l) {
  EGONN_REQUIRE(!gate || (B >= 1 && dense_gate_fusable(n, cin, cout)), EGONN_ERR_INVALID,
                "dense: the fused gated residual needs the LDS-staged kernel (%lld rows, %d->%d)", (long long)n, cin, cout);
  *l = dense_launch(n, cin, cout, form, gate ? B : 0);
  EGONN_REQUIRE(l->route != DENSE_INVALID, EGONN_ERR_INVALID, "dense: no streaming form for %lld rows, %d->%d", (long long)n, cin, cout);
  return EGONN_OK;
}
template <int WOI, int CI, bool INB>
static int dense_lds_launch(const DenseCall& c, const DenseLaunch& l, int io, hipStream_t stream) {
  static AttrOnce attr_done;
  if (attr_done.need()) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_lds_kernel<WOI, CI, INB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024));
    attr_done.mark();
  }
  hipLaunchKernelGGL((dense_lds_kernel<WOI, CI, INB>), dim3(l.gx, l.gy), dim3(256), l.lds, stream, c.in, c.n, c.W, c.cout, c.bias, c.scale,
                     c.shift, c.act, c.residual, c.out, io, c.n_dev, l.colblk, c.gate, c.boff, c.B);
  return EGONN_OK;
}

int dense_forward(const DenseCall& c, hipStream_t stream) {
  if (c.n == 0) return EGONN_OK;
  DenseLaunch l;
  EGONN_TRY(dense_plan(c.n, c.cin, c.cout, c.form, c.gate != nullptr, (c.residual && c.boff) ? c.B : 0, &l));
  const dim3 grid(l.gx, l.gy), block(256);
  const int io = (c.res_bf16 ? 1 : 0) | (c.out_bf16 ? 2 : 0);
  int rc = EGONN_OK;
  switch (l.route) {
    case DENSE_STREAM:
      pick_cin(c.cin, [&](auto CI) { pick<64, 128>(c.cout, [&](auto CO) { pick<0, 1>(c.in_bf16 != 0, [&](auto INB) {
        pick<0, 1>(c.act != ACT_NONE && c.act != ACT_RELU, [&](auto ANY) {
          if constexpr (dense_stream_plan(CI, CO))
            hipLaunchKernelGGL((dense_stream_kernel<CI, CO, INB != 0, ANY != 0>), grid, block, l.lds, stream, c.in, c.n, c.W, c.w_out_in,
                               c.wfrag, c.bias, c.scale, c.shift, c.act, c.residual, c.out, io, c.n_dev, c.gate, c.boff, c.B);
        }); }); }); });
      break;
    case DENSE_LDS:
      dense_dispatch(c, [&](auto CI, auto WOI, auto INB) { rc = dense_lds_launch<WOI, CI, INB>(c, l, io, stream); });
      break;
    case DENSE_SMALL:
    case DENSE_TILE:      // one signature, one grid
      dense_dispatch(c, [&](auto CI, auto WOI, auto INB) {
        auto kernel = &dense_kernel<WOI, CI, INB>;
        if constexpr (CI <= DENSE_SMALL_MAX_CIN)
          if (l.route == DENSE_SMALL) kernel = &dense_small_kernel<WOI, CI, INB>;
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, c.in, c.n, c.W, c.cout, c.bias, c.scale, c.shift, c.act, c.residual, c.out, io, c.n_dev);
      });
      break;
    case DENSE_PLAIN:
      EGONN_REQUIRE(!c.scale && !c.shift && !c.residual && !c.in_bf16 && !c.out_bf16, EGONN_ERR_INVALID, "dense: cin=%d has no fused epilogue",
                    c.cin);
      hipLaunchKernelGGL(dense_any_kernel, grid, block, 0, stream, reinterpret_cast<const float*>(c.in), c.n * c.cout, c.cin, c.W, c.w_out_in,
                         c.cout, c.bias, c.act, reinterpret_cast<float*>(c.out), c.n_dev);
      break;
    default: break;      // (DENSE_NONE and DENSE_INVALID returned above)
  }
  EGONN_TRY(rc);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// Three (n_i, 128) @ (128, 128) products ((cin, cout) kernels, no bias / BN / activation) in ONE launch of dense_small3_kernel;
// fp32 rows in and out.
// wfrag (nullable, all three or none): the same kernels in fragment order (dense_pack_frags) — read instead of W.
bool dense_group3_rows(int64_t n) { return n == 0 || dense_route(n, 128, 128, -1) == DENSE_SMALL; }
int dense_small_group3(const float* const* in, const int64_t* n, const int32_t* const* n_dev, const float* const* W,
                       const float* const* wfrag, float* const* out, hipStream_t stream) {
  const bool packed = wfrag && wfrag[0] && wfrag[1] && wfrag[2];
  DenseGroup3 g;
  int bx = 0;
  for (int q = 0; q < 3; ++q) {
    EGONN_REQUIRE(dense_group3_rows(n[q]), EGONN_ERR_INVALID, "dense(group): %lld rows", (long long)n[q]);
    g.in[q] = in[q]; g.W[q] = packed ? wfrag[q] : W[q]; g.out[q] = out[q]; g.n_dev[q] = n_dev[q]; g.n[q] = n[q];
    g.bx0[q] = bx;
    bx += (int)cdiv(std::max<int64_t>(n[q], 1), 64);
  }
  g.bx0[3] = bx;
  if (packed) hipLaunchKernelGGL((dense_small3_kernel<2, 128, false>), dim3((unsigned)bx, 2), dim3(256), 0, stream, g, 128, 0);
  else hipLaunchKernelGGL((dense_small3_kernel<0, 128, false>), dim3((unsigned)bx, 2), dim3(256), 0, stream, g, 128, 0);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn

using namespace egonn;

// ------------------------------------------------------------------ entry points
// out = act(x @ W + bias) of a stand-alone Linear / 1x1 layer (W in ME kernel or nn.Linear layout)
API int egonn_dense(const float* x, int64_t n, int cin, const float* weight, int weight_out_in, const float* bias, int cout,
                    int act, float* out, void* stream) {
  EGONN_REQUIRE(x && weight && out && n >= 0 && cin >= 1 && cout >= 1 && act >= 0 && act <= 4, EGONN_ERR_INVALID,
                "dense: bad arguments");
  return dense_forward({.in = x, .n = n, .cin = cin, .cout = cout, .W = weight, .w_out_in = weight_out_in ? 1 : 0, .bias = bias, .act = act,
                        .out = out},
                       (hipStream_t)stream);
}
// 1x1 kernels in fragment order
API int egonn_dense_pack_fragments(const float* weight, int weight_out_in, int cin, int cout, float* packed, void* stream) {
  return dense_pack_frags(weight, weight_out_in, cin, cout, packed, (hipStream_t)stream);
}
API int egonn_dense_pack_fragments_host(const float* weight, int weight_out_in, int cin, int cout, float* packed) {
  EGONN_REQUIRE(weight && packed && cin >= 16 && cin % 16 == 0 && cout >= 16 && cout % 16 == 0, EGONN_ERR_INVALID,
                "dense pack: %d->%d (multiples of 16 expected)", cin, cout);
  for (int64_t j = 0; j < (int64_t)cin * cout; ++j) packed[j] = weight[dense_frag_src(j, weight_out_in ? 1 : 0, cin, cout)];
  return EGONN_OK;
}
// the dense launcher with everything explicit
API int egonn_debug_dense(const void* in, int in_bf16, int64_t rows_capacity, const int32_t* n_dev, int cin, int cout, const float* weight,
                          int weight_out_in, const float* packed, const float* bias, const float* scale, const float* shift, int act,
                          const void* residual, int res_bf16, const float* gate, const int32_t* boff, int B, void* out, int out_bf16,
                          int form, void* stream) {
  EGONN_REQUIRE(in && weight && out && rows_capacity >= 0 && cin >= 1 && cout >= 1 && act >= 0 && act <= 4 && (form == 0 || form == 1) &&
                    (!scale == !shift) && (form == 1 || !packed),
                EGONN_ERR_INVALID, "debug_dense: bad arguments");
  return dense_forward({.in = in, .in_bf16 = in_bf16 ? 1 : 0, .n = rows_capacity, .n_dev = n_dev, .cin = cin, .cout = cout, .W = weight,
                        .w_out_in = weight_out_in ? 1 : 0, .wfrag = packed, .bias = bias, .scale = scale, .shift = shift, .act = act,
                        .residual = residual, .res_bf16 = res_bf16 ? 1 : 0, .gate = gate, .boff = boff, .B = B, .out = out,
                        .out_bf16 = out_bf16 ? 1 : 0, .form = form},
                       (hipStream_t)stream);
}
// the grouped lateral launch on the caller's three problems (tests/test_gpu_global_tail.py): packed = all NULL reads the raw kernels
API int egonn_debug_dense_group3(const float* const in[3], const int64_t rows_capacity[3], const int32_t* const n_dev[3],
                                 const float* const weight[3], const float* const packed[3], float* const out[3], void* stream) {
  EGONN_REQUIRE(in && rows_capacity && n_dev && weight && packed && out, EGONN_ERR_INVALID, "debug_dense_group3: null argument");
  for (int q = 0; q < 3; ++q) {
    EGONN_REQUIRE(in[q] && n_dev[q] && weight[q] && out[q] && rows_capacity[q] >= 0 && !packed[q] == !packed[0], EGONN_ERR_INVALID,
                  "debug_dense_group3: bad arguments of problem %d", q);
    EGONN_REQUIRE(dense_group3_rows(rows_capacity[q]), EGONN_ERR_INVALID, "debug_dense_group3: %lld rows are not a small launch",
                  (long long)rows_capacity[q]);
  }
  return dense_small_group3(in, rows_capacity, n_dev, weight, packed, out, (hipStream_t)stream);
}
// what dense_forward would launch for a shape — no device call: out = route (DenseRoute), grid x, grid y, dynamic LDS bytes, colblk
API int egonn_debug_dense_route(int64_t rows, int cin, int cout, int form, int gate_scans, int32_t out[5]) {
  EGONN_REQUIRE(out && rows >= 0 && cin >= 1 && cout >= 1 && form >= -1 && form <= 1 && gate_scans >= 0, EGONN_ERR_INVALID,
                "debug_dense_route: bad arguments");
  DenseLaunch l;
  if (rows > 0) EGONN_TRY(dense_plan(rows, cin, cout, form, gate_scans > 0, gate_scans, &l));
  out[0] = l.route; out[1] = (int32_t)l.gx; out[2] = (int32_t)l.gy; out[3] = (int32_t)l.lds; out[4] = l.colblk;
  return EGONN_OK;
}
