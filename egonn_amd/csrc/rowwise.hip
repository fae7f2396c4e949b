// Row-wise element kernels of the forward: folded BatchNorm, row gather, per-sample column sums, the ECA gate and its
// application, bf16 -> fp32, add, GeM / pool finish and L2 normalisation.
//
// Reference call sites: MinkowskiBatchNorm (nn.BatchNorm1d eval) ; ECALayer layers/eca_block.py:11-36 ; GeM layers/pooling.py:82-86 ;
// MinkowskiFunctional.normalize models/minkgl.py:223.
#include "common.h"
#include "kernels.h"
#include "rowmath.h"

namespace egonn {

// ------------------------------------------------------------------ BatchNorm folding (eval mode)
__global__ void bn_fold_kernel(const float* __restrict__ w, const float* __restrict__ b,
                               const float* __restrict__ rm, const float* __restrict__ rv, float eps, int c,
                               float* __restrict__ scale, float* __restrict__ shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  const float s = w[i] / sqrtf(rv[i] + eps);
  scale[i] = s;
  shift[i] = b[i] - rm[i] * s;
}
int bn_fold(const float* w, const float* b, const float* rm, const float* rv, float eps, int c, float* scale,
            float* shift, hipStream_t stream) {
  hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)cdiv(c, 128)), dim3(128), 0, stream, w, b, rm, rv, eps, c, scale,
                     shift);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ row gather (features -> sorted row order)
__global__ void gather_rows_kernel(const float* __restrict__ in, const int32_t* __restrict__ perm, int64_t n, int c,
                                   float* __restrict__ out, const int32_t* __restrict__ n_dev) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n_dev) n = min((int64_t)*n_dev, n);
  if (t >= n * c) return;
  const int64_t r = t / c;
  const int ch = (int)(t - r * c);
  out[t] = in[(int64_t)perm[r] * c + ch];
}
int gather_rows(const float* in, const int32_t* perm, int64_t n, int c, float* out, hipStream_t stream, const int32_t* n_dev) {
  if (n == 0) return EGONN_OK;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)cdiv(n * c, 256)), dim3(256), 0, stream, in, perm, n, c, out, n_dev);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ per-sample column sums (deterministic)
// grid (SEG_CHUNKS, B): block (ch, b) sums rows [s + ch*len/CH, s + (ch+1)*len/CH) of sample b.
__global__ __launch_bounds__(256) void segment_partial_kernel(const float* __restrict__ in,
                                                               const int32_t* __restrict__ boff, int c, int pow_mode,
                                                               const float* __restrict__ pexp,
                                                               float* __restrict__ partial) {
  __shared__ float red[256];
  const int b = blockIdx.y, ch = blockIdx.x;
  const int32_t s = boff[b], e = boff[b + 1];
  const int64_t len = e - s;
  const int32_t r0 = s + (int32_t)(len * ch / SEG_CHUNKS), r1 = s + (int32_t)(len * (ch + 1) / SEG_CHUNKS);
  const int tid = threadIdx.x;
  const float p = pow_mode == 1 ? pexp[0] : 1.f;           // pow_mode: 0 = sum, 1 = sum of clamp(x)^p (GeM), 2 = max (MAC)
  // c <= 256: thread -> (row lane, channel); for c < 256 several rows advance in parallel
  const int rl = tid / c, cidx = tid - rl * c, nrl = 256 / c;
  float acc = pow_mode == 2 ? -INFINITY : 0.f;
  if (rl < nrl) {
    for (int32_t r = r0 + rl; r < r1; r += nrl) {
      float v = in[(int64_t)r * c + cidx];
      if (pow_mode == 1) v = powf(fmaxf(v, 1e-6f), p);
      acc = pow_mode == 2 ? fmaxf(acc, v) : acc + v;
    }
  }
  red[tid] = acc;
  __syncthreads();
  if (tid < c) {
    float sum = pow_mode == 2 ? -INFINITY : 0.f;
    for (int k = 0; k < nrl; ++k) sum = pow_mode == 2 ? fmaxf(sum, red[k * c + tid]) : sum + red[k * c + tid];
    partial[((int64_t)b * SEG_CHUNKS + ch) * c + tid] = sum;
  }
}
int segment_partial_sums(const float* in, const int32_t* boff, int B, int c, int pow_mode, const float* p,
                         float* partial, hipStream_t stream) {
  EGONN_REQUIRE(c >= 1 && c <= 256 && 256 % c == 0, EGONN_ERR_INVALID, "segment sums: %d channels unsupported", c);
  hipLaunchKernelGGL(segment_partial_kernel, dim3(SEG_CHUNKS, B), dim3(256), 0, stream, in, boff, c, pow_mode, p,
                     partial);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ ECA: gate = sigmoid(conv1d_k(mean)) ; out = relu(x*gate + res)
__global__ void eca_gate_kernel(const float* __restrict__ partial, const int32_t* __restrict__ boff, int c,
                                const float* __restrict__ wconv, int ksize, float* __restrict__ gate) {
  extern __shared__ float mean[];
  const int b = blockIdx.x, t = threadIdx.x;
  const int32_t cntr = boff[b + 1] - boff[b];
  if (t < c) {
    float s = 0.f;
    for (int ch = 0; ch < SEG_CHUNKS; ++ch) s += partial[((int64_t)b * SEG_CHUNKS + ch) * c + t];
    mean[t] = cntr > 0 ? s / (float)cntr : 0.f;
  }
  __syncthreads();
  if (t < c) {
    const int pad = (ksize - 1) / 2;
    float y = 0.f;
    for (int j = 0; j < ksize; ++j) {
      const int q = t + j - pad;
      if (q >= 0 && q < c) y += wconv[j] * mean[q];
    }
    gate[(int64_t)b * c + t] = 1.f / (1.f + expf(-y));
  }
}


// thread = 16 bytes of a row (4 fp32 or 8 bf16 channels): full-width accesses for both precisions (8-byte accesses run at
// 0.5-0.7 of the 16-byte rate); cq = channels / (16 bytes' worth) is a power of two
template <bool BF16>
__global__ void eca_apply_kernel(const void* __restrict__ x, const void* __restrict__ res,
                                 const float* __restrict__ gate, const int32_t* __restrict__ boff, int B, int64_t n,
                                 int cq_shift, void* __restrict__ out) {
  constexpr int CPT = BF16 ? 8 : 4;                      // channels per thread
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  n = min((int64_t)boff[B], n);                          // rows in use (reserved plans size the grid for the capacity)
  if (t >= (n << cq_shift)) return;
  const int32_t r = (int32_t)(t >> cq_shift);
  const int q = (int)(t - ((int64_t)r << cq_shift));
  const int b = sample_of_row(boff, B, r);
  const float* gp = gate + (((int64_t)b << cq_shift) + q) * CPT;
  float xv[CPT], rv[CPT], g[CPT];
  if constexpr (BF16) {
    const uint4 xh = reinterpret_cast<const uint4*>(x)[t], rh = reinterpret_cast<const uint4*>(res)[t];
    const uint32_t xw[4] = {xh.x, xh.y, xh.z, xh.w}, rw[4] = {rh.x, rh.y, rh.z, rh.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xv[2 * i] = bf2f(xw[i] & 0xFFFFu); xv[2 * i + 1] = bf2f(xw[i] >> 16);
      rv[2 * i] = bf2f(rw[i] & 0xFFFFu); rv[2 * i + 1] = bf2f(rw[i] >> 16);
    }
    const float4 g0 = reinterpret_cast<const float4*>(gp)[0], g1 = reinterpret_cast<const float4*>(gp)[1];
    g[0] = g0.x; g[1] = g0.y; g[2] = g0.z; g[3] = g0.w; g[4] = g1.x; g[5] = g1.y; g[6] = g1.z; g[7] = g1.w;
  } else {
    const float4 xf = reinterpret_cast<const float4*>(x)[t], rf = reinterpret_cast<const float4*>(res)[t];
    const float4 g0 = reinterpret_cast<const float4*>(gp)[0];
    xv[0] = xf.x; xv[1] = xf.y; xv[2] = xf.z; xv[3] = xf.w;
    rv[0] = rf.x; rv[1] = rf.y; rv[2] = rf.z; rv[3] = rf.w;
    g[0] = g0.x; g[1] = g0.y; g[2] = g0.z; g[3] = g0.w;
  }
  float o[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) o[i] = fmaxf(xv[i] * g[i] + rv[i], 0.f);
  if constexpr (BF16) {
    uint4 oh;
    oh.x = f2bf_rn(o[0]) | (f2bf_rn(o[1]) << 16);
    oh.y = f2bf_rn(o[2]) | (f2bf_rn(o[3]) << 16);
    oh.z = f2bf_rn(o[4]) | (f2bf_rn(o[5]) << 16);
    oh.w = f2bf_rn(o[6]) | (f2bf_rn(o[7]) << 16);
    reinterpret_cast<uint4*>(out)[t] = oh;
  } else {
    reinterpret_cast<float4*>(out)[t] = make_float4(o[0], o[1], o[2], o[3]);
  }
}
__global__ void bf16_to_f32_kernel(const uint16_t* __restrict__ in, int64_t n, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = bf2f(in[t]);
}
int convert_bf16_to_f32(const void* in, int64_t n, float* out, hipStream_t stream) {
  if (n == 0) return EGONN_OK;
  hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream,
                     reinterpret_cast<const uint16_t*>(in), n, out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

int eca_apply(const float* x, const float* res, const float* partial, const int32_t* boff, int B, int64_t n, int c,
              const float* wconv, int ksize, float* out, hipStream_t stream) {
  EGONN_REQUIRE(c >= 4 && c <= 256 && c % 4 == 0, EGONN_ERR_INVALID, "eca: %d channels unsupported (4..256, multiple of 4)", c);
  if (n == 0) return EGONN_OK;
  // gate lives right behind the partial sums: partial[B*SEG_CHUNKS*c] | gate[B*c]
  float* gate = const_cast<float*>(partial) + (int64_t)B * SEG_CHUNKS * c;
  hipLaunchKernelGGL(eca_gate_kernel, dim3(B), dim3(256), c * sizeof(float), stream, partial, boff, c, wconv, ksize,
                     gate);
  const int c4 = c / 4;
  EGONN_REQUIRE((c4 & (c4 - 1)) == 0, EGONN_ERR_INVALID, "eca_apply: %d channels (a power of two expected)", c);
  hipLaunchKernelGGL(eca_apply_kernel<false>, dim3((unsigned)cdiv(n * c4, 256)), dim3(256), 0, stream, x, res, gate, boff, B,
                     n, __builtin_ctz(c4), out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ECA gate straight from the per-group column sums of the conv2 epilogue (sconv.hip): the groups of sample b are
// rg.meta[1+b] .. rg.meta[2+b] (a window never straddles two samples), summed in fixed order => deterministic.
__global__ __launch_bounds__(1024) void eca_gate_groups_kernel(const float* __restrict__ psum,
                                                                const uint32_t* __restrict__ gmask,
                                                                const int32_t* __restrict__ meta,
                                                                const int32_t* __restrict__ boff, int c,
                                                                const float* __restrict__ wconv, int ksize,
                                                                float* __restrict__ gate) {
  __shared__ float red[1024];
  __shared__ float mean[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int g0 = meta[1 + b], g1 = meta[2 + b];
  const int32_t cntr = boff[b + 1] - boff[b];
  const int nsl = 1024 / c, sl = tid / c, ch = tid - sl * c;    // c <= 256, power of two: 4..32 slices of groups
  // fixed order per slice; the loads of 8 groups are in flight together, and the sums are read whether or not the group
  // is flagged (the buffer covers every group; an unflagged group's value is dropped by the select): with the load behind
  // the flag every group cost two dependent round trips, 16 us for the 800 groups per scan of level 1.
  float acc = 0.f;
  {
    constexpr int U = 8;
    int g = g0 + sl;
    for (; g + (U - 1) * nsl < g1; g += U * nsl) {
      float v[U];
      uint32_t m[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        m[u] = gmask[g + u * nsl];
        v[u] = psum[(int64_t)(g + u * nsl) * c + ch];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) acc += (m[u] >> 31) ? v[u] : 0.f;
    }
    for (; g < g1; g += nsl) {
      const uint32_t m = gmask[g];
      const float v = psum[(int64_t)g * c + ch];
      acc += (m >> 31) ? v : 0.f;
    }
  }
  red[tid] = acc;
  __syncthreads();
  if (tid < c) {
    float s = 0.f;
    for (int k = 0; k < nsl; ++k) s += red[k * c + tid];
    mean[tid] = cntr > 0 ? s / (float)cntr : 0.f;
  }
  __syncthreads();
  if (tid < c) {
    const int pad = (ksize - 1) / 2;
    float y = 0.f;
    for (int j = 0; j < ksize; ++j) {
      const int q = tid + j - pad;
      if (q >= 0 && q < c) y += wconv[j] * mean[q];
    }
    gate[(int64_t)b * c + tid] = 1.f / (1.f + expf(-y));
  }
}
int eca_gate_groups(const float* psum, const RowGroups& rg, const int32_t* boff, int B, int c, const float* wconv, int ksize,
                    float* gate, hipStream_t stream) {
  EGONN_REQUIRE(c >= 32 && c <= 256 && 256 % c == 0, EGONN_ERR_INVALID, "eca gate: %d channels unsupported", c);
  hipLaunchKernelGGL(eca_gate_groups_kernel, dim3(B), dim3(1024), 0, stream, psum, rg.gmask, rg.meta, boff, c, wconv, ksize,
                     gate);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
int eca_apply_gate(const void* x, const void* res, const float* gate, const int32_t* boff, int B, int64_t n, int c,
                   void* out, int bf16, hipStream_t stream) {
  if (n == 0) return EGONN_OK;
  const int cq = bf16 ? c / 8 : c / 4;                   // 16-byte pieces per row
  EGONN_REQUIRE(cq >= 1 && (cq & (cq - 1)) == 0, EGONN_ERR_INVALID, "eca_apply: %d channels (a power of two expected)", c);
  if (bf16)
    hipLaunchKernelGGL(eca_apply_kernel<true>, dim3((unsigned)cdiv(n * cq, 256)), dim3(256), 0, stream, x, res, gate, boff, B, n,
                       __builtin_ctz(cq), out);
  else
    hipLaunchKernelGGL(eca_apply_kernel<false>, dim3((unsigned)cdiv(n * cq, 256)), dim3(256), 0, stream, x, res, gate, boff, B, n,
                       __builtin_ctz(cq), out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

__global__ void add_act_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n, int relu,
                               float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float v = a[t] + b[t];
  out[t] = relu ? fmaxf(v, 0.f) : v;
}
int add_act(const float* a, const float* b, int64_t n, int relu, float* out, hipStream_t stream) {
  if (n == 0) return EGONN_OK;
  hipLaunchKernelGGL(add_act_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, a, b, n, relu, out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ GeM finish
// pexp != NULL: GeM (mean^(1/p)); pexp == NULL: mode 0 = SPoC (mean, MinkowskiGlobalAvgPooling), 2 = MAC (max)
__global__ void gem_finish_kernel(const float* __restrict__ partial, const int32_t* __restrict__ boff, int c,
                                  const float* __restrict__ pexp, int mode, float* __restrict__ out) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (t >= c) return;
  const int32_t cntr = boff[b + 1] - boff[b];
  if (mode == 2) {
    float s = -INFINITY;
    for (int ch = 0; ch < SEG_CHUNKS; ++ch) s = fmaxf(s, partial[((int64_t)b * SEG_CHUNKS + ch) * c + t]);
    out[(int64_t)b * c + t] = cntr > 0 ? s : 0.f;
    return;
  }
  float s = 0.f;
  for (int ch = 0; ch < SEG_CHUNKS; ++ch) s += partial[((int64_t)b * SEG_CHUNKS + ch) * c + t];
  const float m = cntr > 0 ? s / (float)cntr : 0.f;
  out[(int64_t)b * c + t] = pexp ? powf(m, 1.f / pexp[0]) : m;
}
int gem_finish(const float* partial, const int32_t* boff, int B, int c, const float* p, float* out,
               hipStream_t stream) {
  EGONN_REQUIRE(c >= 1 && c <= 256, EGONN_ERR_INVALID, "gem: %d channels unsupported (1..256)", c);
  hipLaunchKernelGGL(gem_finish_kernel, dim3(B), dim3(256), 0, stream, partial, boff, c, p, 0, out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

int pool_finish(const float* partial, const int32_t* boff, int B, int c, int mode, float* out, hipStream_t stream) {
  EGONN_REQUIRE(c >= 1 && c <= 256 && (mode == 0 || mode == 2), EGONN_ERR_INVALID, "pooling: bad arguments");
  hipLaunchKernelGGL(gem_finish_kernel, dim3(B), dim3(256), 0, stream, partial, boff, c, (const float*)nullptr, mode, out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ row L2 normalisation (F.normalize eps=1e-12)
__global__ void l2norm_kernel(float* __restrict__ x, int64_t n, int c, const int32_t* __restrict__ n_dev) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (n_dev) n = min((int64_t)*n_dev, n);
  if (row >= n) return;
  float* p = x + row * c;
  float ss = 0.f;
  for (int i = lane; i < c; i += 64) ss += p[i] * p[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
  for (int i = lane; i < c; i += 64) p[i] *= inv;
}
int l2_normalize_rows(float* x, int64_t n, int c, hipStream_t stream, const int32_t* n_dev) {
  if (n == 0) return EGONN_OK;
  hipLaunchKernelGGL(l2norm_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, stream, x, n, c, n_dev);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn
