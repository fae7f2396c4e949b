// NetVLAD / NetVLAD-GC global pooling of MinkLoc (eval mode), exact fp32 (v_mfma_f32_16x16x4_f32 and FMA, fp32 accumulate).
//
// Reference: NetVLADWrapper layers/pooling.py:89-109 (cluster_size 64, add_batch_norm=True), NetVLADLoupe
// layers/netvlad.py:18-80, GatingContext layers/netvlad.py:83-112.  Per scan b with rows X_b (n_b x C):
//   A       = softmax_k(bn1(X_b @ Wc))                    Wc = cluster_weights (C, 64), bn1 folded to scale/shift
//   a_sum_k = sum_rows A[r,k]  +  (Nmax - n_b) * softmax_k(bn1_shift)
//   V[c,k]  = sum_rows X[r,c] A[r,k] - a_sum_k W2[c,k]     W2 = cluster_weights2 (1, C, 64)
//   vlad    = normalize(normalize_c(V)[c*64 + k])          F.normalize, eps 1e-12 (per cluster, then global)
//   y       = bn2(vlad @ H)                                H = hidden1_weights (C*64, D)
//   gating: y = y * sigmoid(bn_g(y @ Wg))                 Wg = context_gating.gating_weights (D, D)
// Pad rule: the reference zero-pads every scan to Nmax = max_b n_b (pad_sequence, layers/pooling.py:103).  A zero row has
// logits bn1(0) = shift, so each pad row adds softmax(shift) to a_sum and nothing to X^T A: the term above reproduces it.
// Nmax is read from the plan's device-side row offsets (no host synchronisation).
//
// Four launches, no atomics, fixed summation orders (bitwise reproducible, batch-invariant):
//   1. assign + aggregate, grid (NV_MAX_CHUNKS, B): chunk ch of scan b covers rows [n_b*ch/nch, n_b*(ch+1)/nch) with
//      nch = nv_chunks(n_b) (a function of the scan's own row count only); partial X^T A (C x 64) and a_sum per chunk
//   2. finish, grid (C/16, B): chunk sums in chunk order, pad term, - a_sum W2, per-cluster squared norms of 16 c each
//   3. projection, grid (C, ceil(B/16)): the norms -> per-(b,k) scale, then the 64 rows c*64..c*64+63 of H against the
//      scaled V of 16 scans: partial y per c (split-K over C)
//   4. tail, grid B: sum of the C partials (four interleaved parts, combined in order), bn2, (gating GEMM, bn, sigmoid, product)
#include "common.h"
#include "kernels.h"
#include "split16.h"

namespace egonn {

static constexpr int NV_BB = 16;            // scans per workgroup of launch 3

// ------------------------------------------------------------------ 1. assign + aggregate
// Workgroup = 4 waves; wave w owns clusters 16w..16w+15.  Per tile of R = 16*RB rows (staged in LDS, row stride C+4 so that
// both operand reads below are free of bank conflicts for C % 64 == 0):
//   logits: lane (h = lane>>4, c16 = lane&15) feeds A = X[16q + c16][4s + h], B = Wc[4s + h][16w + c16] and ends with
//           logits[16q + 4h + j][16w + c16] in register j of accumulator q;
//   softmax over the 64 clusters: max / sum inside the wave (16 lanes) and across the 4 waves through LDS;
//   X^T A:  the contraction index of MFMA (q, j) is the row 16q + 4h + j, so lane feeds A = X[16q+4h+j][16cb + c16] and its
//           own probability as B: the accumulator of c-block cb holds V[16cb + 4h + j][16w + c16].
template <int MAXCB, int RB>
__global__ __launch_bounds__(256) void netvlad_assign_kernel(const float* __restrict__ x, const int32_t* __restrict__ boff,
                                                             int C, const float* __restrict__ wc,
                                                             const float* __restrict__ sc1, const float* __restrict__ sh1,
                                                             float* __restrict__ part) {
  extern __shared__ float lds[];
  constexpr int R = 16 * RB;
  const int Cp = C + 4;
  float* xs = lds;               // [R][Cp]
  float* red = lds + R * Cp;     // [2][4][R]: row max / row sum per wave
  const int b = blockIdx.y, ch = blockIdx.x;
  const int32_t s0 = boff[b], len = boff[b + 1] - s0;
  const int nch = nv_chunks(len);
  if (ch >= nch) return;
  const int32_t r0 = s0 + (int32_t)((int64_t)len * ch / nch), r1 = s0 + (int32_t)((int64_t)len * (ch + 1) / nch);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, h = lane >> 4, c16 = lane & 15;
  const int k = 16 * w + c16;
  const float scale = sc1[k], shift = sh1[k];
  const int ncb = C >> 4, C4 = C >> 2;
  f32x4 accv[MAXCB];
#pragma unroll
  for (int cb = 0; cb < MAXCB; ++cb) accv[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  // C <= 256: the wave's B operands of the logits product (Wc[4s + h][k], s < C/4) stay in registers for all tiles
  constexpr bool WREG = MAXCB <= 16;
  float wreg[WREG ? 4 * MAXCB : 1];
#pragma unroll
  for (int s = 0; s < (WREG ? 4 * MAXCB : 0); ++s) wreg[s] = s < C4 ? wc[(4 * s + h) * NV_K + k] : 0.f;
  float asum = 0.f;
  for (int32_t t0 = r0; t0 < r1; t0 += R) {
    for (int i = tid; i < R * C4; i += 256) {
      const int rr = i / C4, cc = (i - rr * C4) * 4;
      const int32_t gr = t0 + rr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gr < r1) v = *reinterpret_cast<const float4*>(x + (int64_t)gr * C + cc);
      *reinterpret_cast<float4*>(xs + rr * Cp + cc) = v;
    }
    __syncthreads();
    f32x4 lg[RB];
#pragma unroll
    for (int q = 0; q < RB; ++q) lg[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (WREG) {
#pragma unroll
      for (int s = 0; s < 4 * MAXCB; ++s)
        if (s < C4)
#pragma unroll
          for (int q = 0; q < RB; ++q)
            lg[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[(16 * q + c16) * Cp + 4 * s + h], wreg[s], lg[q], 0, 0, 0);
    } else {
      for (int s = 0; s < C4; ++s) {
        const float bw = wc[(4 * s + h) * NV_K + k];
#pragma unroll
        for (int q = 0; q < RB; ++q)
          lg[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[(16 * q + c16) * Cp + 4 * s + h], bw, lg[q], 0, 0, 0);
      }
    }
    // bn1 (folded) and the row max over the wave's 16 clusters
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float z = lg[q][j] * scale + shift;
        lg[q][j] = z;
        float m = z;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (c16 == 0) red[w * R + 16 * q + 4 * h + j] = m;
      }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 16 * q + 4 * h + j;
        const float m = fmaxf(fmaxf(red[row], red[R + row]), fmaxf(red[2 * R + row], red[3 * R + row]));
        const float e = expf(lg[q][j] - m);
        lg[q][j] = e;
        float sm = e;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sm += __shfl_xor(sm, o, 64);
        if (c16 == 0) red[(4 + w) * R + row] = sm;
      }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 16 * q + 4 * h + j;
        const float sm = ((red[4 * R + row] + red[5 * R + row]) + red[6 * R + row]) + red[7 * R + row];
        const float a = t0 + row < r1 ? lg[q][j] / sm : 0.f;
        lg[q][j] = a;
        asum += a;
      }
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* xr = xs + (16 * q + 4 * h + j) * Cp + c16;
#pragma unroll
        for (int cb = 0; cb < MAXCB; ++cb)
          if (cb < ncb) accv[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[16 * cb], lg[q][j], accv[cb], 0, 0, 0);
      }
    __syncthreads();
  }
  float* P = part + ((int64_t)b * NV_MAX_CHUNKS + ch) * ((int64_t)C * NV_K + NV_K);
#pragma unroll
  for (int cb = 0; cb < MAXCB; ++cb)
    if (cb < ncb)
#pragma unroll
      for (int j = 0; j < 4; ++j) P[(16 * cb + 4 * h + j) * NV_K + k] = accv[cb][j];
  asum += __shfl_xor(asum, 16, 64);
  asum += __shfl_xor(asum, 32, 64);
  if (h == 0) P[C * NV_K + k] = asum;
}

// ------------------------------------------------------------------ 2. finish: V = sum of chunks - a_sum W2
__global__ __launch_bounds__(256) void netvlad_finish_kernel(const float* __restrict__ part, const int32_t* __restrict__ boff,
                                                             int B, int C, const float* __restrict__ w2,
                                                             const float* __restrict__ sh1, float* __restrict__ vraw,
                                                             float* __restrict__ sq) {
  __shared__ float s_asum[NV_K];
  __shared__ float s_red[4][NV_K];
  __shared__ int s_max[256];
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  int mx = 0;
  for (int i = tid; i < B; i += 256) mx = max(mx, boff[i + 1] - boff[i]);
  s_max[tid] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_max[tid] = max(s_max[tid], s_max[tid + o]);
    __syncthreads();
  }
  const int nmax = s_max[0];
  const int32_t nb = boff[b + 1] - boff[b];
  const int nch = nv_chunks(nb);
  const int64_t stride = (int64_t)C * NV_K + NV_K;
  const float* P = part + (int64_t)b * NV_MAX_CHUNKS * stride;
  if (tid < NV_K) {
    // softmax over the clusters of a zero (pad) row: bn1(0) = shift
    const float v = sh1[tid];
    float m = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const float e = expf(v - m);
    float sm = e;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
    float a = 0.f;
    for (int ch = 0; ch < nch; ++ch) a += P[ch * stride + (int64_t)C * NV_K + tid];
    s_asum[tid] = a + (float)(nmax - nb) * (e / sm);
  }
  __syncthreads();
  const int kk = tid & (NV_K - 1);
  const int e0 = (16 * p + (tid >> 6)) * NV_K + kk;      // elements e0 + 4*64*i, i < 4
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int ch = 0; ch < nch; ++ch)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += P[ch * stride + e0 + 4 * NV_K * i];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = e0 + 4 * NV_K * i;
    const float t = v[i] - s_asum[kk] * w2[e];
    vraw[(int64_t)b * C * NV_K + e] = t;
    ss += t * t;
  }
  s_red[tid >> 6][kk] = ss;
  __syncthreads();
  if (tid < NV_K)
    sq[((int64_t)b * (C >> 4) + p) * NV_K + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

// ------------------------------------------------------------------ 3. projection (split-K over c)
// workgroup (c, scan block): per scan the per-cluster and global norms from the squared-norm partials, then
// ppart[c][b][d] = sum_k vlad[b][c*64 + k] * H[c*64 + k][d]
template <int ND>
__global__ __launch_bounds__(256) void netvlad_project_kernel(const float* __restrict__ vraw, const float* __restrict__ sq,
                                                              int B, int C, const float* __restrict__ H, int D,
                                                              float* __restrict__ ppart) {
  __shared__ float s_scale[NV_BB][NV_K];
  __shared__ float s_coef[NV_BB][NV_K];
  __shared__ float s_g[NV_BB];
  const int c = blockIdx.x, b0 = blockIdx.y * NV_BB, tid = threadIdx.x;
  const int nb = min(NV_BB, B - b0), P = C >> 4;
  for (int i = tid; i < NV_BB * NV_K; i += 256) {
    const int bb = i / NV_K, kk = i % NV_K;
    float n2 = 0.f;
    if (bb < nb)
      for (int p = 0; p < P; ++p) n2 += sq[((int64_t)(b0 + bb) * P + p) * NV_K + kk];
    const float nk = sqrtf(n2), inv = 1.f / fmaxf(nk, 1e-12f);
    s_scale[bb][kk] = inv;
    s_coef[bb][kk] = (nk * inv) * (nk * inv);
  }
  __syncthreads();
  if (tid < NV_BB) {
    float g2 = 0.f;
    for (int kk = 0; kk < NV_K; ++kk) g2 += s_coef[tid][kk];
    s_g[tid] = 1.f / fmaxf(sqrtf(g2), 1e-12f);
  }
  __syncthreads();
  for (int i = tid; i < NV_BB * NV_K; i += 256) {
    const int bb = i / NV_K, kk = i % NV_K;
    s_coef[bb][kk] = bb < nb ? vraw[(int64_t)(b0 + bb) * C * NV_K + c * NV_K + kk] * s_scale[bb][kk] * s_g[bb] : 0.f;
  }
  __syncthreads();
  float acc[ND][NV_BB];
#pragma unroll
  for (int j = 0; j < ND; ++j)
#pragma unroll
    for (int bb = 0; bb < NV_BB; ++bb) acc[j][bb] = 0.f;
  const float* Hc = H + (int64_t)c * NV_K * D;
  for (int k0 = 0; k0 < NV_K; k0 += 8) {
    float hv[8][ND];                       // the 8 rows' loads are issued before their FMAs
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int j = 0; j < ND; ++j) {
        const int d = tid + 256 * j;
        hv[u][j] = d < D ? Hc[(int64_t)(k0 + u) * D + d] : 0.f;
      }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int j = 0; j < ND; ++j)
#pragma unroll
        for (int bb = 0; bb < NV_BB; ++bb) acc[j][bb] = fmaf(s_coef[bb][k0 + u], hv[u][j], acc[j][bb]);
  }
#pragma unroll
  for (int j = 0; j < ND; ++j) {
    const int d = tid + 256 * j;
    if (d >= D) continue;
#pragma unroll
    for (int bb = 0; bb < NV_BB; ++bb)
      if (bb < nb) ppart[((int64_t)c * B + b0 + bb) * D + d] = acc[j][bb];
  }
}

// ------------------------------------------------------------------ 4. tail: reduce, bn2, context gating
// 1024 threads: thread (part = tid / 256, d) sums the partials c = part, part + 4, ... ; the four parts combine in order
__global__ __launch_bounds__(1024) void netvlad_tail_kernel(const float* __restrict__ ppart, int B, int C, int D,
                                                            const float* __restrict__ sc2, const float* __restrict__ sh2,
                                                            const float* __restrict__ wg, const float* __restrict__ scg,
                                                            const float* __restrict__ shg, int gating, float* __restrict__ out) {
  __shared__ float red[4][1024];
  __shared__ float ys[1024];
  const int b = blockIdx.x, tid = threadIdx.x, part = tid >> 8;
  for (int d = tid & 255; d < D; d += 256) {
    float y = 0.f;
#pragma unroll 8
    for (int c = part; c < C; c += 4) y += ppart[((int64_t)c * B + b) * D + d];
    red[part][d] = y;
  }
  __syncthreads();
  for (int d = tid; d < D; d += 1024) {
    const float y = (((red[0][d] + red[1][d]) + red[2][d]) + red[3][d]) * sc2[d] + sh2[d];
    ys[d] = y;
    if (!gating) out[(int64_t)b * D + d] = y;
  }
  if (!gating) return;
  __syncthreads();
  for (int d = tid; d < D; d += 1024) {
    float g = 0.f;
#pragma unroll 8
    for (int i = 0; i < D; ++i) g = fmaf(ys[i], wg[(int64_t)i * D + d], g);
    g = g * scg[d] + shg[d];
    out[(int64_t)b * D + d] = ys[d] * (1.f / (1.f + expf(-g)));
  }
}

// ------------------------------------------------------------------ launcher
size_t netvlad_workspace_floats(int B, int C, int D) {
  const size_t part = (size_t)B * NV_MAX_CHUNKS * ((size_t)C * NV_K + NV_K);
  const size_t vraw = (size_t)B * C * NV_K, sq = (size_t)B * (C / 16) * NV_K, pp = (size_t)C * B * D;
  return part + vraw + sq + pp + 4 * 64;      // + alignment slack of the four carve-outs
}

template <int MAXCB, int RB>
static int launch_assign(const float* x, const int32_t* boff, int B, int C, const float* wc, const float* sc1,
                         const float* sh1, float* part, hipStream_t stream) {
  const size_t lds = ((size_t)16 * RB * (C + 4) + 8 * 16 * RB) * sizeof(float);
  static AttrOnce attr;
  if (attr.need()) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&netvlad_assign_kernel<MAXCB, RB>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr.mark();
  }
  hipLaunchKernelGGL((netvlad_assign_kernel<MAXCB, RB>), dim3(NV_MAX_CHUNKS, B), dim3(256), lds, stream, x, boff, C, wc,
                     sc1, sh1, part);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

void netvlad_workspace_carve(float* ws, int B, int C, float** part, float** vraw, float** sq, float** pp) {
  *part = ws;
  *vraw = *part + align_up((size_t)B * NV_MAX_CHUNKS * ((size_t)C * NV_K + NV_K), 64);
  *sq = *vraw + align_up((size_t)B * C * NV_K, 64);
  *pp = *sq + align_up((size_t)B * (C / 16) * NV_K, 64);
}

int netvlad_forward(const float* x, const int32_t* boff, int B, int C, const float* wc, const float* w2, const float* sc1,
                    const float* sh1, const float* H, int D, const float* sc2, const float* sh2, const float* wg,
                    const float* scg, const float* shg, int gating, float* out, float* ws, hipStream_t stream) {
  EGONN_REQUIRE(C >= 16 && C <= 512 && C % 16 == 0 && D >= 16 && D <= 1024 && D % 16 == 0 && B >= 1, EGONN_ERR_INVALID,
                "netvlad: unsupported sizes C=%d D=%d B=%d", C, D, B);
  float *part, *vraw, *sq, *pp;
  netvlad_workspace_carve(ws, B, C, &part, &vraw, &sq, &pp);
  if (C <= 64) EGONN_TRY((launch_assign<4, 4>(x, boff, B, C, wc, sc1, sh1, part, stream)));
  else if (C <= 128) EGONN_TRY((launch_assign<8, 4>(x, boff, B, C, wc, sc1, sh1, part, stream)));
  else if (C <= 256) EGONN_TRY((launch_assign<16, 4>(x, boff, B, C, wc, sc1, sh1, part, stream)));
  else EGONN_TRY((launch_assign<32, 2>(x, boff, B, C, wc, sc1, sh1, part, stream)));
  hipLaunchKernelGGL(netvlad_finish_kernel, dim3(C / 16, B), dim3(256), 0, stream, part, boff, B, C, w2, sh1, vraw, sq);
  HIP_CHECK(hipGetLastError());
  const dim3 pg(C, (B + NV_BB - 1) / NV_BB);
  switch ((D + 255) / 256) {
    case 1: hipLaunchKernelGGL(netvlad_project_kernel<1>, pg, dim3(256), 0, stream, vraw, sq, B, C, H, D, pp); break;
    case 2: hipLaunchKernelGGL(netvlad_project_kernel<2>, pg, dim3(256), 0, stream, vraw, sq, B, C, H, D, pp); break;
    case 3: hipLaunchKernelGGL(netvlad_project_kernel<3>, pg, dim3(256), 0, stream, vraw, sq, B, C, H, D, pp); break;
    default: hipLaunchKernelGGL(netvlad_project_kernel<4>, pg, dim3(256), 0, stream, vraw, sq, B, C, H, D, pp); break;
  }
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(netvlad_tail_kernel, dim3(B), dim3(1024), 0, stream, pp, B, C, D, sc2, sh2, wg, scg, shg, gating, out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn
