// Train-mode pooling of MinkLoc: NetVLAD / NetVLAD-GC forward on batch statistics and its backward, MAC with its argmax,
// the gate product of the context gating.  Exact fp32 (v_mfma_f32_16x16x4_f32 and FMA, fp32 accumulate), BatchNorm sums fp64.
//
// Reference: NetVLADLoupe.forward in .train() under NetVLADWrapper (layers/netvlad.py:44-80, layers/pooling.py:97-109): the
// scans are zero-padded to Nmax = max_b n_b rows and bn1 normalises the logits Z = X Wc of all M = B * Nmax rows.  A pad row has
// Z = 0, so with the sums over the real rows only
//   mean = (sum z) / M,  var = (sum z^2) / M - mean^2       (formed around the running mean in fp64, as BatchNormFn does)
// and every pad row has the logits beta - mean * gamma * invstd = the folded shift.  The eval kernels of netvlad.hip therefore
// run unchanged on the batch scale / shift (launches 1-4, bn2 = identity, no gating): y = vlad @ H.  bn2 and the context gating
// work on (B, D) rows and are composed from the differentiable operators in egonn_amd/train.py.
//
// Forward (netvlad_train_forward): Z = X Wc (dense), fp64 column sums of Z, pad rows added, bn1 finalize (count M, running
// statistics), eval launches 1-4, a_sum per scan.  Saved for the backward: Z (N, 64), bn1 (mean, invstd, scale, shift),
// V before the normalisations (B, C, 64), its squared-norm partials, a_sum (B, 64).  Recomputed: A, vlad.
//
// Backward (netvlad_train_backward), dy = d loss / d y (B, D):
//   1. dvlad = dy H^T                                   one wave per row of H, fixed butterfly
//   2. per scan: the two F.normalize backwards (eps 1e-12 clamps) -> dV (B, C, 64); da_sum[k] = - sum_c W2[c,k] dV[c,k]
//   3. dH = sum_b vlad_b (x) dy_b, dW2 = - sum_b a_sum_b (x) dV_b       batch order
//   4. row pass 1 (MFMA), grid (chunks, B): A = softmax(bn1(Z)), dA = X dV_b + da_sum_b, dL = A o (dA - sum_k A dA); A and dL
//      are stored; per-chunk fp64 column sums of dL and dL (z - mean)
//   5. chunk sums in (scan, chunk) order + the (Nmax - n_b) pad rows of each scan (A = softmax(shift), dA = da_sum_b,
//      z - mean = -mean), then bn_bwd_finalize with count M: dZ = a dL + b Z + c, dgamma, dbeta
//   6. row pass 2 (MFMA): dX = [A | dZ] [dV_b ; Wc]^T, dWc = X^T dZ as per-chunk partials
//   7. dWc = sum of the partials in (scan, chunk) order
// No atomics; every summation order is a function of the scan's own row count (nv_chunks) and, for the sums over scans, of the
// batch order.  A scan's rows of dX depend on the other scans only through the (64,) bn1 vectors and Nmax.
#include "model.h"
#include "split16.h"

namespace egonn {

// ------------------------------------------------------------------ forward helpers
// the pad rows' share of the shifted sums: d = 0 - m for each of `pads` rows
__global__ void nvt_pad_stats_kernel(double* __restrict__ sums, const float* __restrict__ m, double pads) {
  const int k = threadIdx.x;
  const double d = -(double)m[k];
  sums[k] += pads * d;
  sums[NV_K + k] += pads * d * d;
}

// a_sum[b][k] exactly as netvlad_finish_kernel forms it (chunk order, then the pad term)
__global__ __launch_bounds__(64) void nvt_asum_kernel(const float* __restrict__ part, const int32_t* __restrict__ boff, int C,
                                                      int nmax, const float* __restrict__ sh1, float* __restrict__ asum) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int32_t nb = boff[b + 1] - boff[b];
  const int nch = nv_chunks(nb);
  const int64_t stride = (int64_t)C * NV_K + NV_K;
  const float* P = part + (int64_t)b * NV_MAX_CHUNKS * stride;
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
  asum[b * NV_K + tid] = a + (float)(nmax - nb) * (e / sm);
}

__global__ void nvt_fill_kernel(float* __restrict__ p, int n, float v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

static size_t nvt_stats_scratch_floats(int64_t N) { return (size_t)4 * NV_K * (size_t)std::max<int64_t>(1024, N / 512 + 2); }

static size_t netvlad_train_forward_floats(int B, int64_t N, int C, int D) {
  return netvlad_workspace_floats(B, C, D) + nvt_stats_scratch_floats(N) + 2 * (size_t)D + 4 * NV_K + 8 * 64;
}

static int netvlad_train_check(egonn_ctx* ctx, int level, int C, int D, int nmax) {
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS, EGONN_ERR_INVALID, "netvlad_train: level %d out of range", level);
  EGONN_REQUIRE(C >= 16 && C <= 512 && C % 16 == 0, EGONN_ERR_INVALID,
                "netvlad_train: %d channels unsupported (multiple of 16, 16..512)", C);
  EGONN_REQUIRE(D >= 16 && D <= 1024 && D % 16 == 0, EGONN_ERR_INVALID,
                "netvlad_train: output_dim %d unsupported (multiple of 16, 16..1024)", D);
  EGONN_REQUIRE(ctx->plan.batch >= 2, EGONN_ERR_INVALID, "netvlad_train: batch statistics need at least 2 scans");
  EGONN_REQUIRE(ctx->plan.lv[level].n >= 1 && nmax >= 1 && (int64_t)nmax * ctx->plan.batch >= ctx->plan.lv[level].n,
                EGONN_ERR_INVALID, "netvlad_train: nmax %d is not the largest scan of the level", nmax);
  return EGONN_OK;
}

// Train-mode NetVLAD core over the rows of `level`: bn1 on the statistics of the M = B * nmax zero-padded rows, y = vlad @ H
// (B, D) BEFORE bn2; what the backward needs goes to the caller's save_* buffers
API int egonn_netvlad_train_forward(egonn_ctx* ctx, int level, const float* x, int C, int nmax, const float* wc, const float* w2,
                                    const float* bn1_w, const float* bn1_b, float eps, float momentum, float* running_mean,
                                    float* running_var, const float* H, int D, float* out, float* save_z, float* save_bn4,
                                    float* save_vraw, float* save_sq, float* save_asum, void* stream) {
  REQUIRE_PLAN(ctx);
  EGONN_TRY(netvlad_train_check(ctx, level, C, D, nmax));
  EGONN_REQUIRE(x && wc && w2 && bn1_w && bn1_b && running_mean && running_var && H && out && save_z && save_bn4 && save_vraw &&
                    save_sq && save_asum,
                EGONN_ERR_INVALID, "netvlad_train_forward: null argument");
  EGONN_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)save_z & 15) == 0, EGONN_ERR_INVALID,
                "netvlad_train_forward: x and save_z must be 16-byte aligned");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int B = ctx->plan.batch;
  const int64_t N = ctx->plan.lv[level].n;
  const int32_t* boff = ctx->plan.lv[level].boff;
  const size_t nws = netvlad_train_forward_floats(B, N, C, D);
  Arena* A;
  EGONN_TRY(claim_work(ctx, nws * 4 + 4096, false, &A));
  WALLOC(float, ws, nws);
  float* nvws = ws;
  float* cs = nvws + align_up(netvlad_workspace_floats(B, C, D), 64);
  const size_t csn = nvt_stats_scratch_floats(N);
  double* sums = reinterpret_cast<double*>(cs + align_up(csn, 64));          // (2, 64) doubles
  float* ones = reinterpret_cast<float*>(sums + 2 * NV_K);
  float* zeros = ones + D;
  const double M = (double)B * (double)nmax;
  EGONN_TRY(dense_forward({.in = x, .n = N, .cin = C, .cout = NV_K, .W = wc, .out = save_z}, st));
  EGONN_TRY(egonn_col_stats(3, save_z, nullptr, nullptr, running_mean, N, NV_K, sums, cs, (int64_t)csn, st));
  hipLaunchKernelGGL(nvt_pad_stats_kernel, dim3(1), dim3(NV_K), 0, st, sums, running_mean, M - (double)N);
  HIP_CHECK(hipGetLastError());
  EGONN_TRY(egonn_bn_train_finalize(sums, running_mean, M, NV_K, bn1_w, bn1_b, eps, momentum, running_mean, running_var,
                                    save_bn4, st));
  hipLaunchKernelGGL(nvt_fill_kernel, dim3((unsigned)cdiv(D, 256)), dim3(256), 0, st, ones, D, 1.f);
  hipLaunchKernelGGL(nvt_fill_kernel, dim3((unsigned)cdiv(D, 256)), dim3(256), 0, st, zeros, D, 0.f);
  HIP_CHECK(hipGetLastError());
  const float* sc1 = save_bn4 + 2 * NV_K;
  const float* sh1 = save_bn4 + 3 * NV_K;
  EGONN_TRY(netvlad_forward(x, boff, B, C, wc, w2, sc1, sh1, H, D, ones, zeros, nullptr, nullptr, nullptr, 0, out, nvws,
                            st));
  float *part, *vraw, *sq, *pp;
  netvlad_workspace_carve(nvws, B, C, &part, &vraw, &sq, &pp);
  HIP_CHECK(hipMemcpyAsync(save_vraw, vraw, (size_t)B * C * NV_K * 4, hipMemcpyDeviceToDevice, st));
  HIP_CHECK(hipMemcpyAsync(save_sq, sq, (size_t)B * (C / 16) * NV_K * 4, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(nvt_asum_kernel, dim3(B), dim3(64), 0, st, part, boff, C, nmax, sh1, save_asum);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ backward 1: dvlad[b][i] = sum_d dy[b][d] H[i][d]
__global__ __launch_bounds__(256) void nvt_dvlad_kernel(const float* __restrict__ dy, const float* __restrict__ H, int B,
                                                        int CK, int D, float* __restrict__ dvl) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + w;
  if (i >= CK) return;
  float hv[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int d = lane + 64 * j;
    hv[j] = d < D ? H[i * D + d] : 0.f;
  }
  for (int b = 0; b < B; ++b) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int d = lane + 64 * j;
      if (d < D) s = fmaf(dy[(int64_t)b * D + d], hv[j], s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) dvl[(int64_t)b * CK + i] = s;
  }
}

// ------------------------------------------------------------------ backward 2: the two normalisations, one workgroup per scan
// u = V / max(n_k, eps) (per cluster), v = u / max(G, eps) (whole descriptor); thread (part = tid / 64, k) walks c = part, part + 16, ..
//   P_k = sum_c u dv, S = <v, dv>, du = (dv - v S) / G, T_k = sum_c u du = (P_k - S Q_k / G) / G, dV = (du - u T_k) / n_k
// a clamped norm (below eps) is a constant divisor: its projection term is dropped, as autograd does for clamp_min
__global__ __launch_bounds__(1024) void nvt_norm_bwd_kernel(const float* __restrict__ vraw, const float* __restrict__ sq,
                                                            const float* __restrict__ dvl, const float* __restrict__ w2, int C,
                                                            float* __restrict__ dV, float* __restrict__ dasum,
                                                            float* __restrict__ sinv, float* __restrict__ sG) {
  __shared__ float s_inv[NV_K], s_Q[NV_K], s_P[NV_K];
  __shared__ int s_kclamp[NV_K];
  __shared__ float s_red[16][NV_K];
  __shared__ float s_invG, s_S;
  __shared__ int s_gclamp;
  const int b = blockIdx.x, tid = threadIdx.x, k = tid & (NV_K - 1), part = tid >> 6;
  const int P16 = C >> 4;
  const int64_t CK = (int64_t)C * NV_K;
  const float* vb = vraw + b * CK;
  const float* gb = dvl + b * CK;
  if (tid < NV_K) {
    float n2 = 0.f;
    for (int p = 0; p < P16; ++p) n2 += sq[((int64_t)b * P16 + p) * NV_K + k];
    const float nk = sqrtf(n2), inv = 1.f / fmaxf(nk, 1e-12f);
    s_inv[k] = inv;
    s_kclamp[k] = nk < 1e-12f;
    s_Q[k] = (nk * inv) * (nk * inv);
  }
  __syncthreads();
  if (tid == 0) {
    float g2 = 0.f;
    for (int kk = 0; kk < NV_K; ++kk) g2 += s_Q[kk];
    const float G = sqrtf(g2);
    s_invG = 1.f / fmaxf(G, 1e-12f);
    s_gclamp = G < 1e-12f;
  }
  __syncthreads();
  const float inv = s_inv[k], invG = s_invG;
  float p = 0.f;
  for (int c = part; c < C; c += 16) p = fmaf(vb[c * NV_K + k] * inv, gb[c * NV_K + k], p);
  s_red[part][k] = p;
  __syncthreads();
  if (tid < NV_K) {
    float P = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) P += s_red[i][k];
    s_P[k] = P;
    float s = P;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (tid == 0) s_S = s * invG;
    sinv[b * NV_K + k] = inv;
    if (tid == 0) sG[b] = invG;
  }
  __syncthreads();
  const float S = s_gclamp ? 0.f : s_S;
  const float T = s_kclamp[k] ? 0.f : invG * (s_P[k] - S * invG * s_Q[k]);
  float da = 0.f;
  for (int c = part; c < C; c += 16) {
    const float u = vb[c * NV_K + k] * inv, v = u * invG;
    const float du = (gb[c * NV_K + k] - v * S) * invG;
    const float d = (du - u * T) * inv;
    dV[b * CK + c * NV_K + k] = d;
    da = fmaf(w2[c * NV_K + k], d, da);
  }
  __syncthreads();
  s_red[part][k] = da;
  __syncthreads();
  if (tid < NV_K) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) a += s_red[i][k];
    dasum[b * NV_K + k] = -a;
  }
}

// ------------------------------------------------------------------ backward 3: dH and dW2 (sums over the scans, batch order)
__global__ __launch_bounds__(256) void nvt_dh_kernel(const float* __restrict__ vraw, const float* __restrict__ sinv,
                                                     const float* __restrict__ sG, const float* __restrict__ dy, int B,
                                                     int64_t CK, int D, float* __restrict__ dH) {
  const int64_t i = blockIdx.x;
  const int d = blockIdx.y * 256 + threadIdx.x, k = (int)(i & (NV_K - 1));
  if (d >= D) return;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const float vl = (vraw[b * CK + i] * sinv[b * NV_K + k]) * sG[b];
    acc = fmaf(vl, dy[(int64_t)b * D + d], acc);
  }
  dH[i * D + d] = acc;
}

__global__ __launch_bounds__(256) void nvt_dw2_kernel(const float* __restrict__ asum, const float* __restrict__ dV, int B,
                                                      int64_t CK, float* __restrict__ dw2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= CK) return;
  const int k = (int)(e & (NV_K - 1));
  float acc = 0.f;
  for (int b = 0; b < B; ++b) acc = fmaf(asum[b * NV_K + k], dV[b * CK + e], acc);
  dw2[e] = -acc;
}

// ------------------------------------------------------------------ backward 4: row pass 1
// The layout of netvlad_assign_kernel: 4 waves, wave w owns clusters 16w..16w+15, lane (h = lane>>4, c16 = lane&15), tiles of
// R = 16*RB rows staged in LDS with row stride C+4.  dA: lane feeds A = X[16q + c16][4s + h], B = dV_b[4s + h][16w + c16] and
// ends with dA[16q + 4h + j][16w + c16] in register j of accumulator q.  The softmax statistics and sum_k A dA cross the waves
// through LDS.
template <int MAXCB, int RB>
__global__ __launch_bounds__(256) void nvt_rows1_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                        const int32_t* __restrict__ boff, int C, const float* __restrict__ dV,
                                                        const float* __restrict__ dasum, const float* __restrict__ bn4,
                                                        float* __restrict__ As, float* __restrict__ dLs,
                                                        double* __restrict__ partd) {
  extern __shared__ float lds[];
  constexpr int R = 16 * RB;
  const int Cp = C + 4;
  float* xs = lds;               // [R][Cp]
  float* red = lds + R * Cp;     // [3][4][R]: row max / row sum / sum_k A dA per wave
  const int b = blockIdx.y, ch = blockIdx.x;
  const int32_t s0 = boff[b], len = boff[b + 1] - s0;
  const int nch = nv_chunks(len);
  if (ch >= nch) return;
  const int32_t r0 = s0 + (int32_t)((int64_t)len * ch / nch), r1 = s0 + (int32_t)((int64_t)len * (ch + 1) / nch);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, h = lane >> 4, c16 = lane & 15;
  const int k = 16 * w + c16;
  const float mean = bn4[k], scale = bn4[2 * NV_K + k], shift = bn4[3 * NV_K + k], das = dasum[b * NV_K + k];
  const float* dVb = dV + (int64_t)b * C * NV_K;
  const int C4 = C >> 2;
  constexpr bool WREG = MAXCB <= 16;
  float wreg[WREG ? 4 * MAXCB : 1];
#pragma unroll
  for (int s = 0; s < (WREG ? 4 * MAXCB : 0); ++s) wreg[s] = s < C4 ? dVb[(4 * s + h) * NV_K + k] : 0.f;
  double s1 = 0.0, s2 = 0.0;
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
        const float bw = dVb[(4 * s + h) * NV_K + k];
#pragma unroll
        for (int q = 0; q < RB; ++q)
          lg[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[(16 * q + c16) * Cp + 4 * s + h], bw, lg[q], 0, 0, 0);
      }
    }
    float zz[RB][4], a[RB][4];
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 16 * q + 4 * h + j;
        const float zv = t0 + row < r1 ? z[(int64_t)(t0 + row) * NV_K + k] : 0.f;
        zz[q][j] = zv;
        const float l = zv * scale + shift;
        a[q][j] = l;
        float m = l;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (c16 == 0) red[w * R + row] = m;
      }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 16 * q + 4 * h + j;
        const float m = fmaxf(fmaxf(red[row], red[R + row]), fmaxf(red[2 * R + row], red[3 * R + row]));
        const float e = expf(a[q][j] - m);
        a[q][j] = e;
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
        const float av = t0 + row < r1 ? a[q][j] / sm : 0.f;
        a[q][j] = av;
        lg[q][j] += das;
        float t = av * lg[q][j];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o, 64);
        if (c16 == 0) red[(8 + w) * R + row] = t;
      }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 16 * q + 4 * h + j;
        const float t = ((red[8 * R + row] + red[9 * R + row]) + red[10 * R + row]) + red[11 * R + row];
        const float dl = a[q][j] * (lg[q][j] - t);
        if (t0 + row < r1) {
          As[(int64_t)(t0 + row) * NV_K + k] = a[q][j];
          dLs[(int64_t)(t0 + row) * NV_K + k] = dl;
          s1 += (double)dl;
          s2 += (double)dl * (double)(zz[q][j] - mean);
        }
      }
    __syncthreads();
  }
  s1 += __shfl_xor(s1, 16, 64);
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 16, 64);
  s2 += __shfl_xor(s2, 32, 64);
  if (h == 0) {
    double* P = partd + ((int64_t)b * NV_MAX_CHUNKS + ch) * 2 * NV_K;
    P[k] = s1;
    P[NV_K + k] = s2;
  }
}

// ------------------------------------------------------------------ backward 5: sums of bn1's backward (chunks, then pad rows)
__global__ __launch_bounds__(64) void nvt_bn1_sums_kernel(const double* __restrict__ partd, const int32_t* __restrict__ boff,
                                                          int B, int nmax, const float* __restrict__ bn4,
                                                          const float* __restrict__ dasum, double* __restrict__ sums) {
  const int k = threadIdx.x;
  const float mean = bn4[k], v = bn4[3 * NV_K + k];
  float m = v;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const float e = expf(v - m);
  float sm = e;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
  const float ap = e / sm;                       // softmax(shift): the assignment of every pad row
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < B; ++b) {
    const int32_t nb = boff[b + 1] - boff[b];
    const int nch = nv_chunks(nb);
    for (int ch = 0; ch < nch; ++ch) {
      const double* P = partd + ((int64_t)b * NV_MAX_CHUNKS + ch) * 2 * NV_K;
      s1 += P[k];
      s2 += P[NV_K + k];
    }
    const float da = dasum[b * NV_K + k];
    float t = ap * da;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    const double dl = (double)(ap * (da - t)), pads = (double)(nmax - nb);
    s1 += pads * dl;
    s2 += pads * dl * (0.0 - (double)mean);
  }
  sums[k] = s1;
  sums[NV_K + k] = s2;
}

// ------------------------------------------------------------------ backward 6: row pass 2
// dZ = a dL + b Z + c in the lane layout of pass 1 (register (q, j) = row 16q + 4h + j, cluster 16w + c16).
//   dWc: as X^T A of netvlad_assign_kernel — the contraction index of MFMA (q, j) is the row, lane feeds A = X[row][16cb + c16]
//        and its own dZ as B; the accumulator of c-block cb holds dWc[16cb + 4h + j][16w + c16]
//   dX:  P = [A | dZ] (R x 128) goes through LDS (row stride 132); wave w owns the c-blocks cb = w, w + 4, ..; lane feeds
//        A = P[16q + c16][4s + h], B = (4s + h < 64 ? dV_b : Wc)[16cb + c16][(4s + h) % 64] and ends with
//        dX[16q + 4h + j][16cb + c16] in register j
template <int MAXCB, int RB>
__global__ __launch_bounds__(256) void nvt_rows2_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                        const float* __restrict__ As, const float* __restrict__ dLs,
                                                        const int32_t* __restrict__ boff, int C, const float* __restrict__ dV,
                                                        const float* __restrict__ wc, const float* __restrict__ bn5,
                                                        float* __restrict__ dx, float* __restrict__ pwc) {
  extern __shared__ float lds[];
  constexpr int R = 16 * RB, PP = 2 * NV_K + 4, NCW = MAXCB / 4;
  const int Cp = C + 4;
  float* xs = lds;               // [R][Cp]
  float* ps = lds + R * Cp;      // [R][PP]
  const int b = blockIdx.y, ch = blockIdx.x;
  const int32_t s0 = boff[b], len = boff[b + 1] - s0;
  const int nch = nv_chunks(len);
  if (ch >= nch) return;
  const int32_t r0 = s0 + (int32_t)((int64_t)len * ch / nch), r1 = s0 + (int32_t)((int64_t)len * (ch + 1) / nch);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, h = lane >> 4, c16 = lane & 15;
  const int k = 16 * w + c16;
  const float cA = bn5[k], cB = bn5[NV_K + k], cC = bn5[2 * NV_K + k];
  const float* dVb = dV + (int64_t)b * C * NV_K;
  const int ncb = C >> 4, C4 = C >> 2;
  f32x4 accw[MAXCB];
#pragma unroll
  for (int cb = 0; cb < MAXCB; ++cb) accw[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int32_t t0 = r0; t0 < r1; t0 += R) {
    for (int i = tid; i < R * C4; i += 256) {
      const int rr = i / C4, cc = (i - rr * C4) * 4;
      const int32_t gr = t0 + rr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gr < r1) v = *reinterpret_cast<const float4*>(x + (int64_t)gr * C + cc);
      *reinterpret_cast<float4*>(xs + rr * Cp + cc) = v;
    }
    float dz[RB][4];
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 16 * q + 4 * h + j;
        float av = 0.f, d = 0.f;
        if (t0 + row < r1) {
          const int64_t e = (int64_t)(t0 + row) * NV_K + k;
          av = As[e];
          d = fmaf(cA, dLs[e], fmaf(cB, z[e], cC));
        }
        dz[q][j] = d;
        ps[row * PP + k] = av;
        ps[row * PP + NV_K + k] = d;
      }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RB; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* xr = xs + (16 * q + 4 * h + j) * Cp + c16;
#pragma unroll
        for (int cb = 0; cb < MAXCB; ++cb)
          if (cb < ncb) accw[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[16 * cb], dz[q][j], accw[cb], 0, 0, 0);
      }
    f32x4 accx[NCW][RB];
#pragma unroll
    for (int ci = 0; ci < NCW; ++ci)
#pragma unroll
      for (int q = 0; q < RB; ++q) accx[ci][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < 2 * NV_K / 4; ++s) {
      const int kk = 4 * s + h;
      const float* src = kk < NV_K ? dVb + kk : wc + (kk - NV_K);
      float bw[NCW];
#pragma unroll
      for (int ci = 0; ci < NCW; ++ci) {
        const int cb = w + 4 * ci;
        bw[ci] = cb < ncb ? src[(16 * cb + c16) * NV_K] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < RB; ++q) {
        const float pa = ps[(16 * q + c16) * PP + kk];
#pragma unroll
        for (int ci = 0; ci < NCW; ++ci)
          accx[ci][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa, bw[ci], accx[ci][q], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ci = 0; ci < NCW; ++ci) {
      const int cb = w + 4 * ci;
      if (cb < ncb)
#pragma unroll
        for (int q = 0; q < RB; ++q)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int32_t gr = t0 + 16 * q + 4 * h + j;
            if (gr < r1) dx[(int64_t)gr * C + 16 * cb + c16] = accx[ci][q][j];
          }
    }
    __syncthreads();
  }
  float* P = pwc + ((int64_t)b * NV_MAX_CHUNKS + ch) * ((int64_t)C * NV_K);
#pragma unroll
  for (int cb = 0; cb < MAXCB; ++cb)
    if (cb < ncb)
#pragma unroll
      for (int j = 0; j < 4; ++j) P[(16 * cb + 4 * h + j) * NV_K + k] = accw[cb][j];
}

// ------------------------------------------------------------------ backward 7: dWc = partials in (scan, chunk) order
__global__ __launch_bounds__(256) void nvt_dwc_kernel(const float* __restrict__ pwc, const int32_t* __restrict__ boff, int B,
                                                      int64_t CK, float* __restrict__ dwc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= CK) return;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const int nch = nv_chunks(boff[b + 1] - boff[b]);
    for (int ch = 0; ch < nch; ++ch) acc += pwc[((int64_t)b * NV_MAX_CHUNKS + ch) * CK + e];
  }
  dwc[e] = acc;
}

// ------------------------------------------------------------------ backward launcher
template <int MAXCB, int RB>
static int launch_rows(const float* x, const float* z, const int32_t* boff, int B, int C, const float* dV, const float* dasum,
                       const float* bn4, float* As, float* dLs, double* partd, int pass, const float* wc, const float* bn5,
                       float* dx, float* pwc, hipStream_t stream) {
  constexpr int R = 16 * RB;
  static AttrOnce attr;
  if (attr.need()) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nvt_rows1_kernel<MAXCB, RB>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&nvt_rows2_kernel<MAXCB, RB>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr.mark();
  }
  if (pass == 1) {
    const size_t lds = ((size_t)R * (C + 4) + 12 * R) * sizeof(float);
    hipLaunchKernelGGL((nvt_rows1_kernel<MAXCB, RB>), dim3(NV_MAX_CHUNKS, B), dim3(256), lds, stream, x, z, boff, C, dV, dasum,
                       bn4, As, dLs, partd);
  } else {
    const size_t lds = ((size_t)R * (C + 4) + (size_t)R * (2 * NV_K + 4)) * sizeof(float);
    hipLaunchKernelGGL((nvt_rows2_kernel<MAXCB, RB>), dim3(NV_MAX_CHUNKS, B), dim3(256), lds, stream, x, z, As, dLs, boff, C, dV,
                       wc, bn5, dx, pwc);
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

static size_t netvlad_train_backward_floats(int B, int64_t N, int C, int D) {
  const size_t CK = (size_t)C * NV_K;
  return 2 * align_up((size_t)B * CK, 64) + 3 * align_up((size_t)B * NV_K, 64) + 2 * align_up((size_t)N * NV_K, 64) +
         2 * ((size_t)B * NV_MAX_CHUNKS * 2 * NV_K + 2 * NV_K) + (size_t)B * NV_MAX_CHUNKS * CK + 8 * 64;
}

API int egonn_netvlad_train_backward(egonn_ctx* ctx, int level, const float* x, int C, int nmax, const float* wc, const float* w2,
                                     const float* bn1_w, const float* H, int D, const float* dy, const float* z, const float* bn4,
                                     const float* vraw, const float* sq, const float* asum, float* dx, float* dwc, float* dw2,
                                     float* bn5, float* dH, void* stream) {
  REQUIRE_PLAN(ctx);
  EGONN_TRY(netvlad_train_check(ctx, level, C, D, nmax));
  EGONN_REQUIRE(x && wc && w2 && bn1_w && H && dy && z && bn4 && vraw && sq && asum && dx && dwc && dw2 && bn5 && dH,
                EGONN_ERR_INVALID, "netvlad_train_backward: null argument");
  EGONN_REQUIRE(((uintptr_t)x & 15) == 0, EGONN_ERR_INVALID, "netvlad_train_backward: x must be 16-byte aligned");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int B = ctx->plan.batch;
  const int64_t N = ctx->plan.lv[level].n;
  const int32_t* boff = ctx->plan.lv[level].boff;
  const size_t nws = netvlad_train_backward_floats(B, N, C, D);
  Arena* A;
  EGONN_TRY(claim_work(ctx, nws * 4 + 4096, false, &A));
  WALLOC(float, ws, nws);
  const int64_t CK = (int64_t)C * NV_K;
  float* dvl = ws;
  float* dV = dvl + align_up((size_t)B * CK, 64);
  float* dasum = dV + align_up((size_t)B * CK, 64);
  float* sinv = dasum + align_up((size_t)B * NV_K, 64);
  float* sG = sinv + align_up((size_t)B * NV_K, 64);
  float* As = sG + align_up((size_t)B * NV_K, 64);
  float* dLs = As + align_up((size_t)N * NV_K, 64);
  double* partd = reinterpret_cast<double*>(dLs + align_up((size_t)N * NV_K, 64));
  double* sums = partd + (size_t)B * NV_MAX_CHUNKS * 2 * NV_K;
  float* pwc = reinterpret_cast<float*>(sums + 2 * NV_K);
  hipLaunchKernelGGL(nvt_dvlad_kernel, dim3((unsigned)cdiv(CK, 4)), dim3(256), 0, st, dy, H, B, (int)CK, D, dvl);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(nvt_norm_bwd_kernel, dim3(B), dim3(1024), 0, st, vraw, sq, dvl, w2, C, dV, dasum, sinv, sG);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(nvt_dh_kernel, dim3((unsigned)CK, (unsigned)cdiv(D, 256)), dim3(256), 0, st, vraw, sinv, sG, dy, B, CK,
                     D, dH);
  hipLaunchKernelGGL(nvt_dw2_kernel, dim3((unsigned)cdiv(CK, 256)), dim3(256), 0, st, asum, dV, B, CK, dw2);
  HIP_CHECK(hipGetLastError());
  for (int pass = 1; pass <= 2; ++pass) {
    if (C <= 64)
      EGONN_TRY((launch_rows<4, 4>(x, z, boff, B, C, dV, dasum, bn4, As, dLs, partd, pass, wc, bn5, dx, pwc, st)));
    else if (C <= 128)
      EGONN_TRY((launch_rows<8, 4>(x, z, boff, B, C, dV, dasum, bn4, As, dLs, partd, pass, wc, bn5, dx, pwc, st)));
    else if (C <= 256)
      EGONN_TRY((launch_rows<16, 4>(x, z, boff, B, C, dV, dasum, bn4, As, dLs, partd, pass, wc, bn5, dx, pwc, st)));
    else
      EGONN_TRY((launch_rows<32, 2>(x, z, boff, B, C, dV, dasum, bn4, As, dLs, partd, pass, wc, bn5, dx, pwc, st)));
    if (pass == 1) {
      hipLaunchKernelGGL(nvt_bn1_sums_kernel, dim3(1), dim3(64), 0, st, partd, boff, B, nmax, bn4, dasum, sums);
      HIP_CHECK(hipGetLastError());
      EGONN_TRY(egonn_bn_backward_finalize(sums, sums, (double)B * (double)nmax, NV_K, bn1_w, bn4, bn4 + NV_K, bn5, st));
    }
  }
  hipLaunchKernelGGL(nvt_dwc_kernel, dim3((unsigned)cdiv(CK, 256)), dim3(256), 0, st, pwc, boff, B, CK, dwc);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ MAC with its argmax, and its backward
// (the winning plan row of every (scan, channel); ties: lowest row; empty scan: 0 and row -1)
// workgroup (64 channels, scan): 4 row quarters in ascending order, strict > inside and between them: a tie goes to the lowest row
__global__ __launch_bounds__(256) void max_argmax_kernel(const float* __restrict__ in, const int32_t* __restrict__ boff, int C,
                                                         float* __restrict__ out, int32_t* __restrict__ rows) {
  __shared__ float sv[4][64];
  __shared__ int32_t si[4][64];
  const int b = blockIdx.y, tid = threadIdx.x, cl = tid & 63, part = tid >> 6, c = blockIdx.x * 64 + cl;
  const int32_t s0 = boff[b], len = boff[b + 1] - s0;
  const int32_t r0 = s0 + (int32_t)((int64_t)len * part / 4), r1 = s0 + (int32_t)((int64_t)len * (part + 1) / 4);
  float best = 0.f;
  int32_t bi = -1;
  if (c < C)
    for (int32_t r = r0; r < r1; ++r) {
      const float v = in[(int64_t)r * C + c];
      if (bi < 0 || v > best) {
        best = v;
        bi = r;
      }
    }
  sv[part][cl] = best;
  si[part][cl] = bi;
  __syncthreads();
  if (part == 0 && c < C) {
#pragma unroll
    for (int p = 1; p < 4; ++p)
      if (si[p][cl] >= 0 && (bi < 0 || sv[p][cl] > best)) {
        best = sv[p][cl];
        bi = si[p][cl];
      }
    out[(int64_t)b * C + c] = bi < 0 ? 0.f : best;        // an empty scan pools to 0, as egonn_global_max_pool
    rows[(int64_t)b * C + c] = bi;
  }
}

__global__ void max_scatter_kernel(const float* __restrict__ grad, const int32_t* __restrict__ rows, int64_t total, int C,
                                   int64_t n, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int32_t r = rows[i];
  if (r >= 0 && r < n) dx[(int64_t)r * C + (int)(i % C)] = grad[i];
}

API int egonn_global_max_pool_argmax(egonn_ctx* ctx, int level, const float* in, int c, float* out, int32_t* rows, void* stream) {
  REQUIRE_PLAN(ctx);
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS && in && out && rows && c >= 1, EGONN_ERR_INVALID,
                "global_max_pool_argmax: bad argument");
  HIP_CHECK(hipSetDevice(ctx->device));
  const int B = ctx->plan.batch;
  if (B == 0) return EGONN_OK;
  hipLaunchKernelGGL(max_argmax_kernel, dim3((unsigned)cdiv(c, 64), B), dim3(256), 0, (hipStream_t)stream, in,
                     ctx->plan.lv[level].boff, c, out, rows);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_global_max_pool_backward(egonn_ctx* ctx, int level, const float* grad, const int32_t* rows, int c, float* dx,
                                       void* stream) {
  REQUIRE_PLAN(ctx);
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS && grad && rows && dx && c >= 1, EGONN_ERR_INVALID,
                "global_max_pool_backward: bad argument");
  HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = ctx->plan.lv[level].n;
  HIP_CHECK(hipMemsetAsync(dx, 0, (size_t)n * c * 4, st));
  const int64_t total = (int64_t)ctx->plan.batch * c;
  if (total == 0 || n == 0) return EGONN_OK;
  hipLaunchKernelGGL(max_scatter_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, grad, rows, total, c, n, dx);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ context gating product: out = y * sigmoid(t)
// grad == nullptr: forward; else dy = grad * s, dt = grad * y * s * (1 - s)
__global__ void sigmoid_gate_kernel(const float* __restrict__ y, const float* __restrict__ t, const float* __restrict__ grad,
                                    int64_t n, float* __restrict__ out, float* __restrict__ dy, float* __restrict__ dt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float s = 1.f / (1.f + expf(-t[i]));
  if (!grad) {
    out[i] = y[i] * s;
    return;
  }
  const float g = grad[i];
  dy[i] = g * s;
  dt[i] = g * y[i] * s * (1.f - s);
}

API int egonn_sigmoid_gate(const float* y, const float* t, const float* grad, int64_t n, float* out, float* dy, float* dt,
                           void* stream) {
  EGONN_REQUIRE(y && t && n >= 0 && (grad ? (dy && dt) : out != nullptr), EGONN_ERR_INVALID, "sigmoid_gate: bad argument");
  if (n == 0) return EGONN_OK;
  hipLaunchKernelGGL(sigmoid_gate_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, y, t, grad, n, out, dy,
                     dt);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn
