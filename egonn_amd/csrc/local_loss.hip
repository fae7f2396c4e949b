// The whole local-head loss of a batch of (anchor, positive) scan pairs in one library call: KeypointCorrLoss
// (reference models/loss.py:32-92) = KeypointLoss (models/loss_utils.py:23-95) + CorrespondenceLoss (:108-139) per pair,
// averaged over the pairs (metrics_mean, :142-154) — the arithmetic of the per-pair driver in egonn_amd/local_loss.py, with
// the loss, every metric and all six input gradients computed on the device in a fixed launch sequence without any host
// synchronisation.  No (n1 x n2) matrix is stored anywhere: the logits exp(beta) * desc1 . desc2^T are evaluated in LDS tiles
// three times (row statistics, d/d desc1 by rows, d/d desc2 by columns) in exact fp32 FMA arithmetic.
//
// Segments: pair p owns rows [off[p], off[p+1]) of every packed array (DEVICE int32 offsets); launch sizes come from the totals
// the caller passes by value, a workgroup finds its (pair, tile) from the offsets.  Every tile, chunk and reduction is laid out
// relative to the START OF ITS PAIR, so a pair's results do not depend on where it sits in the batch (batch invariance), and
// every sum runs in a fixed order (no float atomics; the one atomic is an integer minimum of packed (distance bits, index)
// keys, which is order-independent).  Ties of every search and arg-max go to the lowest index.
//
// Launches: prepare (kp1' = R kp1 + t, key / flag init) -> keypoint searches both ways -> keypoint -> cloud search, cloud
// side split into LL_CLOUD_CHUNK-point chunks over workgroups -> logit row statistics -> per-pair finish (loss + metrics) ->
// batch mean -> [gradients] d/d desc1, d/d desc2, d/d keypoints and sigmas (gathers in fixed partner order).
#include "model.h"

namespace egonn {

namespace {

constexpr int LL_DIM = 128;              // descriptor width the tile kernels are written for
constexpr int LL_OWN = 32;               // descriptor rows a workgroup owns (8 per wave)
constexpr int LL_OTH = 64;               // rows of the other side per step (one per lane)
constexpr int LL_LD = LL_DIM + 4;        // LDS row stride in floats: 16-byte aligned, b128 reads of 16 consecutive rows hit 64 banks
constexpr int LL_KP_SPLIT = 4;           // keypoint tiles of a pair are dealt over this many workgroups per cloud chunk
static_assert(EGONN_LOCAL_LOSS_STATS == LL_STATS, "header and kernels disagree on the stats row");

__device__ __forceinline__ int ll_segment(const int32_t* __restrict__ off, int pairs, int i) {   // off[p] <= i < off[p+1]
  int lo = 0, hi = pairs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// workgroup b -> (pair, tile of `len` rows inside the pair); false: b is past the last tile
__device__ __forceinline__ bool ll_tile(const int32_t* __restrict__ off, int pairs, int len, int b, int& p, int& t) {
  for (p = 0; p < pairs; ++p) {
    const int nt = (off[p + 1] - off[p] + len - 1) / len;
    if (b < nt) { t = b; return true; }
    b -= nt;
  }
  return false;
}

__device__ __forceinline__ int ll_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__device__ __forceinline__ float ll_norm3(float dx, float dy, float dz) { return sqrtf(dx * dx + dy * dy + dz * dz); }

// ------------------------------------------------------------------ prepare
__global__ __launch_bounds__(256) void ll_prepare_kernel(int pairs, const float* __restrict__ kp1, const int32_t* __restrict__ kp_off1,
                                                          int32_t N1, int32_t N2, const float* __restrict__ T,
                                                          float* __restrict__ kp1t, unsigned long long* __restrict__ ckey1,
                                                          unsigned long long* __restrict__ ckey2, int32_t* __restrict__ iscls) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < N1) {
    const float* M = T + 16 * (int64_t)ll_segment(kp_off1, pairs, i);
    const float x = kp1[3 * i], y = kp1[3 * i + 1], z = kp1[3 * i + 2];
    // pc @ m[:3,:3].T + m[:3,3], accumulated left to right like nn_search_kernel
    kp1t[3 * i] = x * M[0] + y * M[1] + z * M[2] + M[3];
    kp1t[3 * i + 1] = x * M[4] + y * M[5] + z * M[6] + M[7];
    kp1t[3 * i + 2] = x * M[8] + y * M[9] + z * M[10] + M[11];
    ckey1[i] = ~0ull;
  } else if (i - N1 < N2) {
    ckey2[i - N1] = ~0ull;
    iscls[i - N1] = 0;
  }
}

// ------------------------------------------------------------------ keypoint <-> keypoint searches
// thread i < N1: nearest kp2 of kp1'_i; thread N1 + j: nearest kp1' of kp2_j.  Serial scan per thread (first minimum = lowest
// index).  Indices are LOCAL to the pair.  tgt = the class of the correspondence term (-1: farther than dist_th).
__global__ __launch_bounds__(256) void ll_kp_search_kernel(int pairs, const float* __restrict__ kp1t, const int32_t* __restrict__ off1,
                                                            const float* __restrict__ kp2, const int32_t* __restrict__ off2,
                                                            int32_t N1, int32_t N2, float dist_th, int32_t* __restrict__ ndx1,
                                                            float* __restrict__ md1, int32_t* __restrict__ tgt,
                                                            int32_t* __restrict__ ndx2, float* __restrict__ md2,
                                                            int32_t* __restrict__ iscls) {
  const int32_t g = blockIdx.x * 256 + threadIdx.x;
  const bool first = g < N1;
  const int32_t i = first ? g : g - N1;
  if (!first && i >= N2) return;
  const float* a = first ? kp1t : kp2;
  const float* b = first ? kp2 : kp1t;
  const int p = ll_segment(first ? off1 : off2, pairs, i);
  const int32_t b0 = first ? off2[p] : off1[p], nb = (first ? off2[p + 1] : off1[p + 1]) - b0;
  const float px = a[3 * i], py = a[3 * i + 1], pz = a[3 * i + 2];
  float best = INFINITY;
  int32_t bi = 0;
  for (int32_t j = 0; j < nb; ++j) {
    const float dx = px - b[3 * (b0 + j)], dy = py - b[3 * (b0 + j) + 1], dz = pz - b[3 * (b0 + j) + 2];
    const float d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < best) { best = d2; bi = j; }
  }
  float d = INFINITY;
  if (nb > 0) {
    const int32_t j = b0 + bi;
    d = first ? ll_norm3(px - b[3 * j], py - b[3 * j + 1], pz - b[3 * j + 2])
              : ll_norm3(b[3 * j] - px, b[3 * j + 1] - py, b[3 * j + 2] - pz);
  }
  if (first) {
    const bool kept = d <= dist_th;
    ndx1[i] = bi; md1[i] = d; tgt[i] = kept ? bi : -1;
    if (kept) iscls[b0 + bi] = 1;        // every writer stores the same value
  } else {
    ndx2[i] = bi; md2[i] = d;
  }
}

// ------------------------------------------------------------------ keypoint -> own cloud search
// workgroup = (cloud chunk of a pair, one of LL_KP_SPLIT shares of the pair's keypoint tiles, side).  The chunk sits in LDS; a
// thread scans it for one keypoint and merges its (squared distance bits, local cloud index) into the keypoint's 64-bit key
// with an integer minimum: smaller distance first, then the lower index, whatever the order the chunks arrive in.
__global__ __launch_bounds__(256) void ll_cloud_search_kernel(int pairs, const float* __restrict__ c1, const int32_t* __restrict__ coff1,
                                                               const float* __restrict__ c2, const int32_t* __restrict__ coff2,
                                                               const float* __restrict__ k1, const int32_t* __restrict__ koff1,
                                                               const float* __restrict__ k2, const int32_t* __restrict__ koff2,
                                                               unsigned long long* __restrict__ key1,
                                                               unsigned long long* __restrict__ key2) {
  __shared__ float sb[LL_CLOUD_CHUNK * 3];
  const bool s2 = blockIdx.z != 0;
  const float* cloud = s2 ? c2 : c1;
  const float* kp = s2 ? k2 : k1;
  const int32_t* coff = s2 ? coff2 : coff1;
  const int32_t* koff = s2 ? koff2 : koff1;
  unsigned long long* key = s2 ? key2 : key1;
  int p, ch;
  if (!ll_tile(coff, pairs, LL_CLOUD_CHUNK, blockIdx.x, p, ch)) return;
  const int32_t c0 = coff[p] + ch * LL_CLOUD_CHUNK, cnt = min(LL_CLOUD_CHUNK, coff[p + 1] - c0);
  const int32_t k0 = koff[p], nk = koff[p + 1] - k0;
  const int tid = threadIdx.x;
  for (int e = tid; e < cnt * 3; e += 256) sb[e] = cloud[(int64_t)c0 * 3 + e];
  __syncthreads();
  for (int32_t i = blockIdx.y * 256 + tid; i < nk; i += LL_KP_SPLIT * 256) {
    const float px = kp[3 * (k0 + i)], py = kp[3 * (k0 + i) + 1], pz = kp[3 * (k0 + i) + 2];
    float best = INFINITY;
    int32_t bi = -1;
    for (int32_t j = 0; j < cnt; ++j) {
      const float dx = px - sb[3 * j], dy = py - sb[3 * j + 1], dz = pz - sb[3 * j + 2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (d2 < best) { best = d2; bi = j; }
    }
    if (bi >= 0)
      atomicMin(&key[k0 + i], ((unsigned long long)__float_as_uint(best) << 32) | (uint32_t)(ch * LL_CLOUD_CHUNK + bi));
  }
}

// ------------------------------------------------------------------ correspondence term on LDS tiles
// logits S[i][j] = scale * desc1_i . desc2_j of one pair, never stored.  A workgroup owns LL_OWN descriptor rows of one side (8
// per wave) and walks the other side in steps of LL_OTH rows (one per lane); a thread accumulates 8 dot products in fp32 FMAs, k
// ascending — the same order in all three modes, so the three evaluations of a logit agree bitwise.
//   MODE 0  owns desc1 rows: online softmax per lane, merged over the wave's lanes in a fixed butterfly -> lse, row loss, arg-max
//           (lowest index), and the maximum of the row with every class column replaced by 0 (the 'neg_similarity' rule)
//   MODE 1  owns desc1 rows: g_desc1_i = sum_j dS_ij desc2_j
//   MODE 2  owns desc2 rows: g_desc2_j = sum_i dS_ij desc1_i
//   dS_ij = coef / K_pair * (exp(S_ij - lse_i) - [j == class_i]) on the kept rows i, 0 elsewhere; sums over the other side
//   ascending.  A pair without a kept row (K = 0) has a NaN loss: its descriptor gradients are NaN, as autograd makes them.
template <int MODE>
__global__ __launch_bounds__(256) void ll_corr_kernel(int pairs, const float* __restrict__ desc1, const float* __restrict__ desc2,
                                                       const int32_t* __restrict__ off1, const int32_t* __restrict__ off2,
                                                       const int32_t* __restrict__ tgt, const int32_t* __restrict__ iscls,
                                                       float scale, float coef, float* __restrict__ lse,
                                                       float* __restrict__ rowloss, int32_t* __restrict__ amax,
                                                       float* __restrict__ negmax, const float* __restrict__ pairK,
                                                       float* __restrict__ gout) {
  __shared__ __attribute__((aligned(16))) float s_own[LL_OWN * LL_LD];
  __shared__ __attribute__((aligned(16))) float s_oth[LL_OTH * LL_LD];
  __shared__ float s_ds[MODE ? LL_OWN * (LL_OTH + 1) : 1];
  const int32_t* offA = MODE == 2 ? off2 : off1;
  const int32_t* offB = MODE == 2 ? off1 : off2;
  const float* A = MODE == 2 ? desc2 : desc1;
  const float* B = MODE == 2 ? desc1 : desc2;
  int p, t;
  if (!ll_tile(offA, pairs, LL_OWN, blockIdx.x, p, t)) return;
  const int32_t a0 = offA[p] + t * LL_OWN, na = min(LL_OWN, offA[p + 1] - a0);
  const int32_t b0 = offB[p], nb = offB[p + 1] - b0;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r2 = tid >> 3, kq = tid & 7;        // accumulation phase of MODE 1 / 2: output row, 4 x 4 columns kq*4 + 32*u

  if (MODE != 0) {
    const float K = pairK[p];
    if (!(K > 0.f)) {
      if (r2 < na)
        for (int u = 0; u < 4; ++u)
          *(float4*)&gout[(int64_t)(a0 + r2) * LL_DIM + u * 32 + kq * 4] = make_float4(NAN, NAN, NAN, NAN);
      return;
    }
    coef = coef / K;
  }
  for (int e = tid; e < LL_OWN * (LL_DIM / 4); e += 256) {
    const int r = e >> 5, k4 = e & 31;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < na) v = ((const float4*)(A + (int64_t)(a0 + r) * LL_DIM))[k4];
    *(float4*)&s_own[r * LL_LD + k4 * 4] = v;
  }
  // MODE 0 state per owned row q of this wave, per lane
  float m[8], s[8], st[8], ng[8];
  int32_t am[8], tg[8];
  float g[16];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    m[q] = -INFINITY; s[q] = 0.f; st[q] = 0.f; ng[q] = -INFINITY; am[q] = 0x7FFFFFFF;
    const int r = w * 8 + q;
    tg[q] = (MODE != 2 && r < na) ? tgt[a0 + r] : -1;
  }
#pragma unroll
  for (int u = 0; u < 16; ++u) g[u] = 0.f;
  float ls[8];                                   // MODE 1: lse of the owned rows
  if (MODE == 1) {
#pragma unroll
    for (int q = 0; q < 8; ++q) ls[q] = tg[q] >= 0 ? lse[a0 + w * 8 + q] : 0.f;
  }

  for (int32_t jt = 0; jt < nb; jt += LL_OTH) {
    __syncthreads();
    for (int e = tid; e < LL_OTH * (LL_DIM / 4); e += 256) {
      const int r = e >> 5, k4 = e & 31;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (jt + r < nb) v = ((const float4*)(B + (int64_t)(b0 + jt + r) * LL_DIM))[k4];
      *(float4*)&s_oth[r * LL_LD + k4 * 4] = v;
    }
    __syncthreads();
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    const float* bp = &s_oth[lane * LL_LD];
    const float* ap = &s_own[(w * 8) * LL_LD];
#pragma unroll 2
    for (int k4 = 0; k4 < LL_DIM / 4; ++k4) {
      const float4 b = *(const float4*)(bp + k4 * 4);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float4 a = *(const float4*)(ap + q * LL_LD + k4 * 4);
        acc[q] = fmaf(a.x, b.x, acc[q]);
        acc[q] = fmaf(a.y, b.y, acc[q]);
        acc[q] = fmaf(a.z, b.z, acc[q]);
        acc[q] = fmaf(a.w, b.w, acc[q]);
      }
    }
    const int32_t j = jt + lane;                 // local index on the other side
    const bool valid = j < nb;
    if (MODE == 0) {
      const bool cls = valid && iscls[b0 + j] != 0;
      if (valid) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float v = scale * acc[q];
          if (v > m[q]) { s[q] = s[q] * expf(m[q] - v) + 1.f; m[q] = v; am[q] = j; }
          else s[q] += expf(v - m[q]);
          if (j == tg[q]) st[q] = v;
          ng[q] = fmaxf(ng[q], cls ? 0.f : v);
        }
      }
    } else {
      float lo = 0.f;
      int32_t to = -1;
      if (MODE == 2 && valid) {                  // the kp1 row is the other side: its class and lse
        to = tgt[b0 + j];
        lo = to >= 0 ? lse[b0 + j] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = w * 8 + q;
        float d = 0.f;
        if (MODE == 1) {
          if (valid && tg[q] >= 0) d = coef * (expf(scale * acc[q] - ls[q]) - (j == tg[q] ? 1.f : 0.f));
        } else {
          const int32_t jl = t * LL_OWN + r;     // local desc2 index of the owned row
          if (valid && r < na && to >= 0) d = coef * (expf(scale * acc[q] - lo) - (jl == to ? 1.f : 0.f));
        }
        s_ds[r * (LL_OTH + 1) + lane] = d;
      }
      __syncthreads();
      const float* dp = &s_ds[r2 * (LL_OTH + 1)];
#pragma unroll 4
      for (int c = 0; c < LL_OTH; ++c) {
        const float d = dp[c];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 b = *(const float4*)&s_oth[c * LL_LD + u * 32 + kq * 4];
          g[u * 4 + 0] = fmaf(d, b.x, g[u * 4 + 0]);
          g[u * 4 + 1] = fmaf(d, b.y, g[u * 4 + 1]);
          g[u * 4 + 2] = fmaf(d, b.z, g[u * 4 + 2]);
          g[u * 4 + 3] = fmaf(d, b.w, g[u * 4 + 3]);
        }
      }
    }
  }

  if (MODE == 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {         // fixed butterfly: both partners compute the same merged state
        const float om = __shfl_xor(m[q], o, 64), os = __shfl_xor(s[q], o, 64);
        const int32_t oa = __shfl_xor(am[q], o, 64);
        const float nm = fmaxf(m[q], om);
        const float e1 = m[q] == -INFINITY ? 0.f : expf(m[q] - nm), e2 = om == -INFINITY ? 0.f : expf(om - nm);
        if (om > m[q] || (om == m[q] && oa < am[q])) am[q] = oa;
        s[q] = s[q] * e1 + os * e2;
        m[q] = nm;
        st[q] += __shfl_xor(st[q], o, 64);       // one lane holds the class logit, the others 0
        ng[q] = fmaxf(ng[q], __shfl_xor(ng[q], o, 64));
      }
      const int r = w * 8 + q;
      if (lane == 0 && r < na) {
        const bool kept = tg[q] >= 0;
        const float l = m[q] + logf(s[q]);
        lse[a0 + r] = kept ? l : 0.f;
        rowloss[a0 + r] = kept ? l - st[q] : 0.f;
        amax[a0 + r] = am[q];
        negmax[a0 + r] = kept ? ng[q] : 0.f;
      }
    }
  } else if (r2 < na) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      *(float4*)&gout[(int64_t)(a0 + r2) * LL_DIM + u * 32 + kq * 4] =
          make_float4(g[u * 4], g[u * 4 + 1], g[u * 4 + 2], g[u * 4 + 3]);
  }
}

// ------------------------------------------------------------------ per-pair loss and metrics
struct LLArgs {
  int pairs;
  int32_t N1, N2, M1, M2;
  const float *c1, *c2, *kp1, *kp2, *s1, *s2, *T;
  const int32_t *coff1, *coff2, *off1, *off2;
  const float* kp1t;
  const int32_t *ndx1, *ndx2, *tgt, *amax;
  const float *md1, *md2, *rowloss, *negmax;
  const unsigned long long *ckey1, *ckey2;
  float gamma_chamfer, gamma_p2p, gamma_c, gamma_k, dist_th;
};

// distance of keypoint row i (global) of a side to the cloud point its search key names; (ux, uy, uz) = kp - point
__device__ __forceinline__ float ll_p2p(const float* __restrict__ kp, int32_t i, const float* __restrict__ cloud, int32_t c0,
                                        int32_t m, int32_t M, unsigned long long key, float& ux, float& uy, float& uz) {
  const int32_t c = ll_clamp(c0 + ll_clamp((int32_t)(uint32_t)(key & 0xFFFFFFFFull), m), M);
  ux = kp[3 * i] - cloud[3 * (int64_t)c];
  uy = kp[3 * i + 1] - cloud[3 * (int64_t)c + 1];
  uz = kp[3 * i + 2] - cloud[3 * (int64_t)c + 2];
  return ll_norm3(ux, uy, uz);
}

constexpr int LL_NQ = 18;

// one workgroup per pair: thread-strided partial sums over the pair's keypoints (local index), then a fixed tree per quantity
__global__ __launch_bounds__(256) void ll_finish_kernel(LLArgs a, float* __restrict__ out_pair, float* __restrict__ pairK) {
  __shared__ float red[256];
  const int p = blockIdx.x, t = threadIdx.x;
  const int32_t o1 = a.off1[p], n1 = a.off1[p + 1] - o1, o2 = a.off2[p], n2 = a.off2[p + 1] - o2;
  const int32_t co1 = a.coff1[p], m1 = a.coff1[p + 1] - co1, co2 = a.coff2[p], m2 = a.coff2[p + 1] - co2;
  float v[LL_NQ];
#pragma unroll
  for (int k = 0; k < LL_NQ; ++k) v[k] = 0.f;
  float ux, uy, uz;
  for (int32_t l = t; l < n1; l += 256) {
    const int32_t i = o1 + l;
    const float md = a.md1[i];
    const float s12 = 0.5f * (a.s1[i] + a.s2[ll_clamp(o2 + a.ndx1[i], a.N2)]);
    v[0] += logf(s12) + md / s12;
    v[1] += md <= a.dist_th ? 1.f : 0.f;
    v[2] += md;
    v[3] += 1.f / s12;
    v[4] += md / s12;
    v[5] += s12;
    v[6] += ll_p2p(a.kp1, i, a.c1, co1, m1, a.M1, a.ckey1[i], ux, uy, uz);
    const int32_t tg = a.tgt[i];
    if (tg >= 0) {
      v[7] += 1.f;
      v[8] += a.rowloss[i];
      v[9] += a.amax[i] == tg ? 1.f : 0.f;
      v[10] += (float)a.amax[i];
      v[11] += a.negmax[i];
    }
  }
  for (int32_t l = t; l < n2; l += 256) {
    const int32_t j = o2 + l;
    const float md = a.md2[j];
    const float s21 = 0.5f * (a.s2[j] + a.s1[ll_clamp(o1 + a.ndx2[j], a.N1)]);
    v[12] += logf(s21) + md / s21;
    v[13] += md;
    v[14] += 1.f / s21;
    v[15] += md / s21;
    v[16] += s21;
    v[17] += ll_p2p(a.kp2, j, a.c2, co2, m2, a.M2, a.ckey2[j], ux, uy, uz);
  }
  for (int k = 0; k < LL_NQ; ++k) {
    __syncthreads();
    red[t] = v[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) red[t] += red[t + o];
      __syncthreads();
    }
    v[k] = red[0];
  }
  if (t == 0) {
    const float f1 = (float)n1, f2 = (float)n2, K = v[7];
    const float loss_ch = a.gamma_chamfer * 0.5f * (v[0] / f1 + v[12] / f2);
    const float p2p = 0.5f * (v[6] / f1 + v[17] / f2);
    const float kl = loss_ch + a.gamma_p2p * p2p;
    const float corr = v[8] / K;                 // K = 0: CrossEntropyLoss over no rows = nan
    float* o = out_pair + (int64_t)p * LL_STATS;
    o[0] = a.gamma_k * kl + a.gamma_c * corr;
    o[1] = 0.5f * (f1 + f2);
    o[2] = v[1] / f1;
    o[3] = 0.5f * (v[2] / f1 + v[13] / f2);
    o[4] = 0.5f * (v[4] / v[3]) + 0.5f * (v[15] / v[14]);
    o[5] = 0.5f * (v[5] / f1 + v[16] / f2);
    o[6] = loss_ch;
    o[7] = p2p;
    o[8] = kl;
    o[9] = corr;
    o[10] = K;
    o[11] = K > 0.f ? v[9] : 0.f;
    o[12] = K > 0.f ? v[10] / K : 0.f;
    o[13] = K > 0.f ? v[11] / K : 0.f;
    o[14] = 0.f;
    o[15] = 0.f;
    pairK[p] = K;
  }
}

__global__ void ll_batch_mean_kernel(int pairs, const float* __restrict__ out_pair, float* __restrict__ out_batch) {
  const int k = threadIdx.x;
  if (k >= LL_STATS) return;
  float s = 0.f;
  for (int p = 0; p < pairs; ++p) s += out_pair[(int64_t)p * LL_STATS + k];
  out_batch[k] = s / (float)pairs;
}

// ------------------------------------------------------------------ gradients to keypoints and sigmas
// thread per keypoint of either side: its own chamfer term, the terms of every partner that selected it (gathered in ascending
// partner order), its point-to-point term.  A zero distance contributes no gradient (torch.cdist's convention).
__global__ __launch_bounds__(256) void ll_point_grad_kernel(LLArgs a, float* __restrict__ g_kp1, float* __restrict__ g_s1,
                                                             float* __restrict__ g_kp2, float* __restrict__ g_s2) {
  const int32_t g = blockIdx.x * 256 + threadIdx.x;
  const bool first = g < a.N1;
  const int32_t i = first ? g : g - a.N1;
  if (!first && i >= a.N2) return;
  const int p = ll_segment(first ? a.off1 : a.off2, a.pairs, i);
  const int32_t o1 = a.off1[p], n1 = a.off1[p + 1] - o1, o2 = a.off2[p], n2 = a.off2[p + 1] - o2;
  const float w = 1.f / (float)a.pairs;
  const float wk = a.gamma_k * a.gamma_chamfer * 0.5f * w, wp = a.gamma_k * a.gamma_p2p * 0.5f * w;
  const float c1 = wk / (float)n1, c2 = wk / (float)n2;
  float gx = 0.f, gy = 0.f, gz = 0.f, gs = 0.f;      // d / d kp1' (first) or d / d kp2
  float ux, uy, uz;
  if (first) {
    const float px = a.kp1t[3 * i], py = a.kp1t[3 * i + 1], pz = a.kp1t[3 * i + 2], si = a.s1[i];
    {
      const int32_t j = ll_clamp(o2 + a.ndx1[i], a.N2);
      const float s12 = 0.5f * (si + a.s2[j]), md = a.md1[i], cs = c1 / s12;
      if (md > 0.f) {
        gx += cs * ((px - a.kp2[3 * j]) / md); gy += cs * ((py - a.kp2[3 * j + 1]) / md); gz += cs * ((pz - a.kp2[3 * j + 2]) / md);
      }
      gs += 0.5f * c1 * (1.f / s12 - md / (s12 * s12));
    }
    const int32_t li = i - o1;
    for (int32_t l = 0; l < n2; ++l) {
      const int32_t j = o2 + l;
      if (a.ndx2[j] != li) continue;
      const float s21 = 0.5f * (a.s2[j] + si), md = a.md2[j], cs = c2 / s21;
      if (md > 0.f) {
        gx += cs * ((px - a.kp2[3 * j]) / md); gy += cs * ((py - a.kp2[3 * j + 1]) / md); gz += cs * ((pz - a.kp2[3 * j + 2]) / md);
      }
      gs += 0.5f * c2 * (1.f / s21 - md / (s21 * s21));
    }
    const float* M = a.T + 16 * (int64_t)p;            // kp1' = R kp1 + t  =>  d/d kp1 = R^T d/d kp1'
    float ox = gx * M[0] + gy * M[4] + gz * M[8], oy = gx * M[1] + gy * M[5] + gz * M[9], oz = gx * M[2] + gy * M[6] + gz * M[10];
    const int32_t co = a.coff1[p];
    const float d = ll_p2p(a.kp1, i, a.c1, co, a.coff1[p + 1] - co, a.M1, a.ckey1[i], ux, uy, uz);
    if (d > 0.f) {
      const float cp = wp / (float)n1;
      ox += cp * (ux / d); oy += cp * (uy / d); oz += cp * (uz / d);
    }
    g_kp1[3 * i] = ox; g_kp1[3 * i + 1] = oy; g_kp1[3 * i + 2] = oz;
    g_s1[i] = gs;
  } else {
    const float qx = a.kp2[3 * i], qy = a.kp2[3 * i + 1], qz = a.kp2[3 * i + 2], sj = a.s2[i];
    {
      const int32_t k = ll_clamp(o1 + a.ndx2[i], a.N1);
      const float s21 = 0.5f * (sj + a.s1[k]), md = a.md2[i], cs = c2 / s21;
      if (md > 0.f) {
        gx -= cs * ((a.kp1t[3 * k] - qx) / md); gy -= cs * ((a.kp1t[3 * k + 1] - qy) / md); gz -= cs * ((a.kp1t[3 * k + 2] - qz) / md);
      }
      gs += 0.5f * c2 * (1.f / s21 - md / (s21 * s21));
    }
    const int32_t lj = i - o2;
    for (int32_t l = 0; l < n1; ++l) {
      const int32_t k = o1 + l;
      if (a.ndx1[k] != lj) continue;
      const float s12 = 0.5f * (a.s1[k] + sj), md = a.md1[k], cs = c1 / s12;
      if (md > 0.f) {
        gx -= cs * ((a.kp1t[3 * k] - qx) / md); gy -= cs * ((a.kp1t[3 * k + 1] - qy) / md); gz -= cs * ((a.kp1t[3 * k + 2] - qz) / md);
      }
      gs += 0.5f * c1 * (1.f / s12 - md / (s12 * s12));
    }
    const int32_t co = a.coff2[p];
    const float d = ll_p2p(a.kp2, i, a.c2, co, a.coff2[p + 1] - co, a.M2, a.ckey2[i], ux, uy, uz);
    if (d > 0.f) {
      const float cp = wp / (float)n2;
      gx += cp * (ux / d); gy += cp * (uy / d); gz += cp * (uz / d);
    }
    g_kp2[3 * i] = gx; g_kp2[3 * i + 1] = gy; g_kp2[3 * i + 2] = gz;
    g_s2[i] = gs;
  }
}

// the carves of the caller's scratch, in this order.  With scratch = nullptr only `total` means anything
struct LLSpan {
  float* kp1t;
  unsigned long long *ckey1, *ckey2;
  int32_t *ndx1, *tgt, *amax, *ndx2, *iscls;
  float *md1, *lse, *rowloss, *negmax, *md2, *pairK;
  size_t total;
};
LLSpan ll_span(void* scratch, int pairs, int64_t n_kp1, int64_t n_kp2) {
  LLSpan S;
  Carve c(scratch);
  const size_t n1 = (size_t)(n_kp1 < 0 ? 0 : n_kp1), n2 = (size_t)(n_kp2 < 0 ? 0 : n_kp2);
  S.kp1t = c.take<float>(n1 * 3);
  S.ckey1 = c.take<unsigned long long>(n1);
  S.ckey2 = c.take<unsigned long long>(n2);
  S.ndx1 = c.take<int32_t>(n1), S.md1 = c.take<float>(n1), S.tgt = c.take<int32_t>(n1), S.lse = c.take<float>(n1);
  S.rowloss = c.take<float>(n1), S.amax = c.take<int32_t>(n1), S.negmax = c.take<float>(n1);
  S.ndx2 = c.take<int32_t>(n2), S.md2 = c.take<float>(n2), S.iscls = c.take<int32_t>(n2);
  S.pairK = c.take<float>((size_t)(pairs < 1 ? 1 : pairs));
  S.total = c.total();
  return S;
}

}  // namespace

API int64_t egonn_local_loss_scratch_bytes(int pairs, int64_t n_kp1, int64_t n_kp2, int dim) {
  (void)dim;
  return (int64_t)ll_span(nullptr, pairs, n_kp1, n_kp2).total;
}

// clouds (M,3), keypoints (N,3) (N) (N,128) and their offsets (pairs+1) on the device, transforms (pairs,16); params on the HOST:
// gamma_chamfer, gamma_p2p, gamma_c, gamma_k, beta, dist_th; out_pair (pairs, LL_STATS), out_batch (LL_STATS); the six gradient
// outputs all null: loss and metrics only
API int egonn_local_loss(int pairs, int64_t n_cloud1, int64_t n_cloud2, int64_t n_kp1, int64_t n_kp2, int dim,
                         const float* clouds1, const int32_t* cloud_off1, const float* clouds2, const int32_t* cloud_off2,
                         const float* kp1, const float* sigma1, const float* desc1, const int32_t* kp_off1,
                         const float* kp2, const float* sigma2, const float* desc2, const int32_t* kp_off2,
                         const float* transforms, const float* params, float* out_pair, float* out_batch,
                         float* g_kp1, float* g_sigma1, float* g_desc1, float* g_kp2, float* g_sigma2, float* g_desc2,
                         void* scratch, int64_t scratch_bytes, void* stream) {
  // every check runs before anything touches the device
  EGONN_REQUIRE(pairs >= 1 && pairs <= 4096, EGONN_ERR_INVALID, "local_loss: pairs=%d outside [1, 4096]", pairs);
  EGONN_REQUIRE(dim == LL_DIM, EGONN_ERR_INVALID, "local_loss: descriptor width %d not supported (128)", dim);
  const int64_t lim = (1ll << 31) / 128;       // row * 128 and cloud row * 3 stay inside int32 / the packed key
  EGONN_REQUIRE(n_cloud1 >= 1 && n_cloud2 >= 1 && n_kp1 >= 1 && n_kp2 >= 1 && n_kp1 < lim && n_kp2 < lim &&
                    n_cloud1 < (1ll << 31) / 3 && n_cloud2 < (1ll << 31) / 3 && n_kp1 + n_kp2 < (1ll << 31) - 256,
                EGONN_ERR_INVALID, "local_loss: totals out of range (clouds %lld %lld, keypoints %lld %lld)",
                (long long)n_cloud1, (long long)n_cloud2, (long long)n_kp1, (long long)n_kp2);
  EGONN_REQUIRE(clouds1 && cloud_off1 && clouds2 && cloud_off2 && kp1 && sigma1 && desc1 && kp_off1 && kp2 && sigma2 && desc2 &&
                    kp_off2 && transforms && params && out_pair && out_batch && scratch,
                EGONN_ERR_INVALID, "local_loss: null argument");
  const int ng = (g_kp1 != nullptr) + (g_sigma1 != nullptr) + (g_desc1 != nullptr) + (g_kp2 != nullptr) + (g_sigma2 != nullptr) +
                 (g_desc2 != nullptr);
  EGONN_REQUIRE(ng == 0 || ng == 6, EGONN_ERR_INVALID, "local_loss: the six gradient outputs are given together or not at all");
  EGONN_REQUIRE((((uintptr_t)desc1 | (uintptr_t)desc2 | (uintptr_t)g_desc1 | (uintptr_t)g_desc2) & 15) == 0 &&
                    ((uintptr_t)scratch & 255) == 0,
                EGONN_ERR_INVALID, "local_loss: descriptors must be 16-byte aligned, scratch 256-byte aligned");
  const LLSpan S = ll_span(scratch, pairs, n_kp1, n_kp2);
  const int64_t need = (int64_t)S.total;
  EGONN_REQUIRE(scratch_bytes >= need, EGONN_ERR_INVALID, "local_loss: scratch of %lld bytes, %lld needed",
                (long long)scratch_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  const int32_t N1 = (int32_t)n_kp1, N2 = (int32_t)n_kp2;
  const float gamma_chamfer = params[0], gamma_p2p = params[1], gamma_c = params[2], gamma_k = params[3];
  const float scale = expf(params[4]), dist_th = params[5];

  const unsigned flat = (unsigned)cdiv((int64_t)N1 + N2, 256);
  hipLaunchKernelGGL(ll_prepare_kernel, dim3(flat), dim3(256), 0, st, pairs, kp1, kp_off1, N1, N2, transforms, S.kp1t,
                     S.ckey1, S.ckey2, S.iscls);
  hipLaunchKernelGGL(ll_kp_search_kernel, dim3(flat), dim3(256), 0, st, pairs, S.kp1t, kp_off1, kp2, kp_off2, N1, N2,
                     dist_th, S.ndx1, S.md1, S.tgt, S.ndx2, S.md2, S.iscls);
  // chunks of a side <= total / chunk + one partial chunk per pair
  const int64_t chunks = cdiv(n_cloud1 > n_cloud2 ? n_cloud1 : n_cloud2, LL_CLOUD_CHUNK) + pairs;
  hipLaunchKernelGGL(ll_cloud_search_kernel, dim3((unsigned)chunks, LL_KP_SPLIT, 2), dim3(256), 0, st, pairs, clouds1,
                     cloud_off1, clouds2, cloud_off2, kp1, kp_off1, kp2, kp_off2, S.ckey1, S.ckey2);
  const unsigned tiles1 = (unsigned)(cdiv(N1, LL_OWN) + pairs), tiles2 = (unsigned)(cdiv(N2, LL_OWN) + pairs);
  hipLaunchKernelGGL(ll_corr_kernel<0>, dim3(tiles1), dim3(256), 0, st, pairs, desc1, desc2, kp_off1, kp_off2, S.tgt,
                     S.iscls, scale, 0.f, S.lse, S.rowloss, S.amax, S.negmax, (const float*)nullptr, (float*)nullptr);
  LLArgs a;
  a.pairs = pairs; a.N1 = N1; a.N2 = N2; a.M1 = (int32_t)n_cloud1; a.M2 = (int32_t)n_cloud2;
  a.c1 = clouds1; a.c2 = clouds2; a.kp1 = kp1; a.kp2 = kp2; a.s1 = sigma1; a.s2 = sigma2; a.T = transforms;
  a.coff1 = cloud_off1; a.coff2 = cloud_off2; a.off1 = kp_off1; a.off2 = kp_off2;
  a.kp1t = S.kp1t; a.ndx1 = S.ndx1; a.ndx2 = S.ndx2; a.tgt = S.tgt; a.amax = S.amax;
  a.md1 = S.md1; a.md2 = S.md2; a.rowloss = S.rowloss; a.negmax = S.negmax; a.ckey1 = S.ckey1; a.ckey2 = S.ckey2;
  a.gamma_chamfer = gamma_chamfer; a.gamma_p2p = gamma_p2p; a.gamma_c = gamma_c; a.gamma_k = gamma_k; a.dist_th = dist_th;
  hipLaunchKernelGGL(ll_finish_kernel, dim3(pairs), dim3(256), 0, st, a, out_pair, S.pairK);
  hipLaunchKernelGGL(ll_batch_mean_kernel, dim3(1), dim3(64), 0, st, pairs, (const float*)out_pair, out_batch);
  if (g_kp1) {
    const float coef = gamma_c * scale / (float)pairs;
    hipLaunchKernelGGL(ll_corr_kernel<1>, dim3(tiles1), dim3(256), 0, st, pairs, desc1, desc2, kp_off1, kp_off2, S.tgt,
                       S.iscls, scale, coef, S.lse, S.rowloss, S.amax, S.negmax, (const float*)S.pairK, g_desc1);
    hipLaunchKernelGGL(ll_corr_kernel<2>, dim3(tiles2), dim3(256), 0, st, pairs, desc1, desc2, kp_off1, kp_off2, S.tgt,
                       S.iscls, scale, coef, S.lse, S.rowloss, S.amax, S.negmax, (const float*)S.pairK, g_desc2);
    hipLaunchKernelGGL(ll_point_grad_kernel, dim3(flat), dim3(256), 0, st, a, g_kp1, g_sigma1, g_kp2, g_sigma2);
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn
