// ScanContext, the hand-crafted baseline the reference measures EgoNN against (third_party/scan_context/scan_context.py,
// evaluate_scan_context.py), on the device: descriptors and ring keys of a resident scan batch, the circular-shift column-cosine
// distance of (query, candidate) pairs, and the rerank of every query's candidate list.
//
// Descriptor (scan_context.py:9-55).  The reference works on float32 arrays, so every step has one float32 meaning:
//     faraway = sqrt(x*x + y*y)                    products, sum and root rounded one by one (np.linalg.norm over an axis)
//     theta   = clip(atan2(y, x) + float32(pi), 0, float32(2 pi - 1e-6))
//     ring    = faraway // float32(max_length / R);   sector = theta // float32(2 pi / S);   ring >= R is dropped
//     cell    = max(0, max over the cell's points of z + float32(lidar_height))
// numpy's float floor-division returns the floor of the EXACT quotient of its two float32 operands (it goes through fmod);
// sc_floor_div does the same with one division and an exact fma remainder.  faraway is therefore bitwise the reference's and
// rings agree for every input; sectors agree wherever atan2f and numpy's float32 arctan2 land in the same sector (they may
// differ in the last bit of theta, which matters only within ~4e-7 rad of a sector edge).  A point with a NaN coordinate, or
// with a ring that is not in [0, R), is dropped; a NaN height counts as 0.
// sc_cells_kernel: grid (G, B): G workgroups per scan, each streams a contiguous share of the scan's rows (three float4 loads
// per lane for four rows where the rows are 16-byte aligned), holds the R x S cells in LDS as the uint32 bit patterns of the
// clamped heights (non-negative floats order like their bit patterns, so an integer atomicMax is exact and independent of
// arrival order) and merges its non-zero cells into the zero-initialised output with a global atomicMax on the same view.
// The result is bitwise deterministic; there is no float atomic anywhere.  Empty cells stay +0.0.
// sc_ringkey_kernel: one wave per (scan, ring) row: the mean over sectors, summed in a fixed order (scan_context.py:86-88).
//
// Distance (scan_context.py:58-83: distance_sc(candidate, query)).  For shift i = 1..S, a = roll(candidate, i) along sectors:
//     sim_i = mean over columns c with |a[:,c]| > 1e-8 and |q[:,c]| > 1e-8 of  a[:,c].q[:,c] / (|a[:,c]| |q[:,c]|)
//     dist = 1 - max_i sim_i,  yaw = (argmax_i + 1) % S with argmax counted from 0 over i = 1..S (first maximum; NaN counts as
//     the maximum, as np.argmax / np.max have it: a shift with no column in common gives 0/0)
// With every column divided by its norm once (masked-out columns set to 0) the numerator of sim_i is a circular
// cross-correlation summed over the rings, and the number of common columns is the same correlation of the two 0/1 masks:
// it rides along as row R.  sc_distance_kernel: grid (ceil(k / KP), Q); a workgroup normalises its query into LDS once, then
// for each of its KP candidates stages the normalised candidate twice side by side (so a rolled read needs no modulo),
// wave w takes rows w, w+4, ..., lane = shift: lanes read consecutive LDS words of the candidate row and four broadcast words
// of the query row per step.  S > 64 gives a lane two shifts.  The four waves' partial sums are added in wave order, and wave
// 0 reduces (max, first index) across lanes.  A pair's arithmetic does not depend on KP or on the list it came from.
//
// Rerank (scan_context.py:151-154): per query a rank sort of its k <= 128 entries by (distance, candidate index, position);
// NaN after every number, as np.argsort has it.
#include "../../include/egonn_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int SC_MAX_RING = 40, SC_MAX_SECTOR = 128, SC_MAX_K = 128;
static constexpr int SC_WG = 256;            // lanes of a descriptor workgroup
static constexpr int SC_ROWS_PER_WG = 2048;  // rows a descriptor workgroup streams when the batch is large enough
static constexpr int SC_MAX_CHUNKS = 128;    // workgroups per scan at most
static constexpr int SCD_WG = 256;           // lanes of a distance workgroup (4 waves)
static constexpr int SCD_MAX_KP = 8;         // candidates a distance workgroup walks through at most

struct ScParams {
  float gap_ring, gap_sector, theta_max, lidar_height;
  int R, S;
};

// floor of the exact quotient a / b of two floats (b > 0): what numpy's floor_divide returns.  The rounded quotient is off by
// far less than 1, so its floor is off by at most 1; the fma remainder a - k b has the sign of the exact one.
__device__ __forceinline__ float sc_floor_div(float a, float b) {
  float k = floorf(__fdiv_rn(a, b));
  const float r = fmaf(-k, b, a);
  if (r < 0.f) k -= 1.f;
  else if (r >= b) k += 1.f;
  return k;
}

__device__ __forceinline__ void sc_point(const ScParams& P, float x, float y, float z, uint32_t* cells) {
  const float faraway = __fsqrt_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)));
  const float kr = sc_floor_div(faraway, P.gap_ring);
  if (!(kr >= 0.f && kr < (float)P.R)) return;               // beyond max_length, or a NaN coordinate
  float th = __fadd_rn(atan2f(y, x), 3.14159274f);
  th = fminf(fmaxf(th, 0.f), P.theta_max);
  int s = (int)sc_floor_div(th, P.gap_sector);
  s = min(max(s, 0), P.S - 1);
  const float h = __fadd_rn(z, P.lidar_height);
  if (h > 0.f) atomicMax(&cells[(int)kr * P.S + s], __float_as_uint(h));     // h <= 0 or NaN: the cell's 0 stands
}

__global__ __launch_bounds__(SC_WG) void sc_cells_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                        int64_t n_cap, ScParams P, int vec4, uint32_t* __restrict__ out) {
  extern __shared__ uint32_t s_cells[];
  const int b = blockIdx.y, t = threadIdx.x;
  const int cells = P.R * P.S;
  for (int i = t; i < cells; i += SC_WG) s_cells[i] = 0u;
  __syncthreads();
  int64_t lo = off[b], hi = off[b + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n_cap ? n_cap : hi;                               // rows beyond the capacity are never read
  if (hi <= lo) return;                                       // an empty scan: its zero-initialised cells stand
  // the scan's rows in groups of four whose first row is a multiple of four, so that a whole group is three aligned float4
  const int64_t g0 = lo >> 2, g1 = (hi + 3) >> 2;
  const int64_t per = (g1 - g0 + gridDim.x - 1) / gridDim.x;
  const int64_t ga = g0 + (int64_t)blockIdx.x * per;
  const int64_t ge = ga + per < g1 ? ga + per : g1;
  for (int64_t g = ga + t; g < ge; g += SC_WG) {
    const int64_t r0 = g * 4;
    if (vec4 && r0 >= lo && r0 + 4 <= hi) {
      const float4* p = reinterpret_cast<const float4*>(pts + r0 * 3);
      const float4 u = p[0], v = p[1], w = p[2];
      sc_point(P, u.x, u.y, u.z, s_cells);
      sc_point(P, u.w, v.x, v.y, s_cells);
      sc_point(P, v.z, v.w, w.x, s_cells);
      sc_point(P, w.y, w.z, w.w, s_cells);
    } else {
      for (int j = 0; j < 4; ++j) {
        const int64_t r = r0 + j;
        if (r >= lo && r < hi) sc_point(P, pts[r * 3], pts[r * 3 + 1], pts[r * 3 + 2], s_cells);
      }
    }
  }
  __syncthreads();
  uint32_t* o = out + (int64_t)b * cells;
  for (int i = t; i < cells; i += SC_WG) {
    const uint32_t v = s_cells[i];
    if (v) atomicMax(&o[i], v);
  }
}

__global__ __launch_bounds__(256) void sc_ringkey_kernel(const float* __restrict__ sc, int64_t rows, int S, float* __restrict__ rk) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float s = 0.f;
  for (int j = lane; j < S; j += 64) s += sc[row * S + j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) rk[row] = s / (float)S;
}

// ------------------------------------------------------------------ distance
// does (b, ib) take the place of (a, ia) as the maximum?  NaN is the maximum; equal values: the lower index
__device__ __forceinline__ bool scd_better(float a, int ia, float b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an != bn) return bn;
  if (!an && a != b) return b > a;
  return ib < ia;
}

// columns of the R x S descriptor at base[r * stride + j] -> 1 / norm per column (0 where the norm is <= 1e-8) in s_inv,
// the 0 / 1 mask in row R
__device__ __forceinline__ void scd_column_norms(float* base, int stride, int R, int S, float* s_inv, int t) {
  if (t < S) {
    float ss = 0.f;
    for (int r = 0; r < R; ++r) {
      const float v = base[r * stride + t];
      ss = fmaf(v, v, ss);
    }
    const float nrm = __fsqrt_rn(ss);
    const bool ok = nrm > 1e-8f;
    s_inv[t] = ok ? __fdiv_rn(1.f, nrm) : 0.f;
    base[R * stride + t] = ok ? 1.f : 0.f;
  }
}

static size_t scd_lds_bytes(int R, int S) {
  const int S4 = (S + 3) & ~3;
  return ((size_t)(R + 1) * S4 * 3 + 4 * SC_MAX_SECTOR + 2 * SC_MAX_SECTOR) * sizeof(float);
}

__global__ __launch_bounds__(SCD_WG) void sc_distance_kernel(const float* __restrict__ qsc, const float* __restrict__ msc,
                                                            const int32_t* __restrict__ cand, int64_t M, int k, int R, int S,
                                                            int KP, float* __restrict__ out_dist, int32_t* __restrict__ out_yaw) {
  extern __shared__ __align__(16) float s_mem[];
  const int S4 = (S + 3) & ~3, C2 = 2 * S4, R1 = R + 1, RS = R * S;
  float* s_q = s_mem;                         // [R1][S4]  normalised query, row R = mask, columns >= S zero
  float* s_c = s_q + R1 * S4;                 // [R1][C2]  normalised candidate at columns j and j + S, the rest zero
  float* s_num = s_c + R1 * C2;               // [4][128]  per-wave numerators
  float* s_cnt = s_num + 4 * SC_MAX_SECTOR;   // [128]     common columns
  float* s_inv = s_cnt + SC_MAX_SECTOR;       // [128]
  const int64_t q = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;

  for (int i = t; i < R1 * S4; i += SCD_WG) s_q[i] = 0.f;
  for (int i = t; i < R1 * C2; i += SCD_WG) s_c[i] = 0.f;
  __syncthreads();
  for (int i = t; i < RS; i += SCD_WG) {
    const int r = i / S, j = i - r * S;
    s_q[r * S4 + j] = qsc[q * RS + i];
  }
  __syncthreads();
  scd_column_norms(s_q, S4, R, S, s_inv, t);
  __syncthreads();
  for (int i = t; i < RS; i += SCD_WG) {
    const int r = i / S, j = i - r * S;
    s_q[r * S4 + j] *= s_inv[j];
  }
  // (the first barrier of the candidate loop orders these writes before the reads)

  const int p0 = blockIdx.x * KP, p1 = min(k, p0 + KP);
  const int l0 = min(lane, S - 1), l1 = min(lane + 64, S - 1);      // lanes without a shift recompute the last one
  for (int p = p0; p < p1; ++p) {
    const int64_t c = cand ? (int64_t)cand[q * k + p] : (int64_t)p;
    if (c < 0 || c >= M) {                                          // uniform over the workgroup
      if (t == 0) {
        out_dist[q * k + p] = INFINITY;
        out_yaw[q * k + p] = -1;
      }
      continue;
    }
    __syncthreads();                                                // the previous candidate's reads are over
    for (int i = t; i < RS; i += SCD_WG) {
      const int r = i / S, j = i - r * S;
      s_c[r * C2 + j] = msc[c * RS + i];
    }
    __syncthreads();
    scd_column_norms(s_c, C2, R, S, s_inv, t);
    __syncthreads();
    for (int i = t; i < R1 * S; i += SCD_WG) {
      const int r = i / S, j = i - r * S;
      const float v = r < R ? s_c[r * C2 + j] * s_inv[j] : s_c[r * C2 + j];
      s_c[r * C2 + j] = v;
      s_c[r * C2 + j + S] = v;
    }
    __syncthreads();

    float num0 = 0.f, num1 = 0.f, cnt0 = 0.f, cnt1 = 0.f;
    for (int r = w; r < R1; r += 4) {
      const float* qa = s_q + r * S4;
      const float* c0 = s_c + r * C2 + (S - 1) - l0;               // c0[col] = candidate column (col - shift) mod S, shift = l0 + 1
      const float* c1 = s_c + r * C2 + (S - 1) - l1;
      float a0 = 0.f, a1 = 0.f;
      for (int col = 0; col < S4; col += 4) {
        const float4 qv = *reinterpret_cast<const float4*>(qa + col);
        a0 = fmaf(qv.x, c0[col], a0);
        a0 = fmaf(qv.y, c0[col + 1], a0);
        a0 = fmaf(qv.z, c0[col + 2], a0);
        a0 = fmaf(qv.w, c0[col + 3], a0);
        if (S > 64) {
          a1 = fmaf(qv.x, c1[col], a1);
          a1 = fmaf(qv.y, c1[col + 1], a1);
          a1 = fmaf(qv.z, c1[col + 2], a1);
          a1 = fmaf(qv.w, c1[col + 3], a1);
        }
      }
      if (r == R) {
        cnt0 = a0;
        cnt1 = a1;
      } else {
        num0 += a0;
        num1 += a1;
      }
    }
    s_num[w * SC_MAX_SECTOR + lane] = num0;
    s_num[w * SC_MAX_SECTOR + 64 + lane] = num1;
    if (w == (R & 3)) {
      s_cnt[lane] = cnt0;
      s_cnt[64 + lane] = cnt1;
    }
    __syncthreads();
    if (w == 0) {
      float best = -INFINITY;
      int bi = 0x7fffffff;
      for (int l = lane; l < S; l += 64) {
        const float tot = ((s_num[l] + s_num[SC_MAX_SECTOR + l]) + s_num[2 * SC_MAX_SECTOR + l]) + s_num[3 * SC_MAX_SECTOR + l];
        const float sim = __fdiv_rn(tot, s_cnt[l]);                 // no common column: 0 / 0 = NaN, as in the reference
        if (scd_better(best, bi, sim, l)) {
          best = sim;
          bi = l;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (scd_better(best, bi, ov, oi)) {
          best = ov;
          bi = oi;
        }
      }
      if (lane == 0) {
        out_dist[q * k + p] = 1.f - best;
        out_yaw[q * k + p] = (bi + 1) % S;
      }
    }
  }
}

// ------------------------------------------------------------------ rerank
__global__ __launch_bounds__(SC_MAX_K) void sc_rerank_kernel(const float* __restrict__ dist, const int32_t* __restrict__ yaw,
                                                            const int32_t* __restrict__ cand, int k, int32_t* __restrict__ out_index,
                                                            float* __restrict__ out_dist, int32_t* __restrict__ out_yaw) {
  __shared__ float s_d[SC_MAX_K];
  __shared__ int32_t s_i[SC_MAX_K];
  const int64_t q = blockIdx.x;
  const int t = threadIdx.x;
  if (t < k) {
    s_d[t] = dist[q * k + t];
    s_i[t] = cand ? cand[q * k + t] : t;
  }
  __syncthreads();
  if (t >= k) return;
  const float d = s_d[t];
  const int32_t c = s_i[t];
  const bool dn = d != d;
  int rank = 0;
  for (int j = 0; j < k; ++j) {
    const float dj = s_d[j];
    const int32_t cj = s_i[j];
    const bool jn = dj != dj;
    bool before;
    if (jn != dn) before = dn;                     // a number comes before NaN
    else if (!dn && dj != d) before = dj < d;
    else if (cj != c) before = cj < c;
    else before = j < t;
    rank += before ? 1 : 0;
  }
  out_index[q * k + rank] = c;
  out_dist[q * k + rank] = d;
  out_yaw[q * k + rank] = yaw[q * k + t];
}

static bool sc_shape_ok(int R, int S) { return R >= 1 && R <= SC_MAX_RING && S >= 2 && S <= SC_MAX_SECTOR; }

}  // namespace egonn

using namespace egonn;

API int egonn_scan_context(const float* points, int64_t n, const int64_t* scan_offsets, int batch_size, int num_sector,
                           int num_ring, double max_length, double lidar_height, float* out_sc, float* out_ringkey,
                           void* stream) {
  EGONN_REQUIRE(sc_shape_ok(num_ring, num_sector), EGONN_ERR_INVALID,
                "scan_context: num_ring %d outside [1, %d] or num_sector %d outside [2, %d]", num_ring, SC_MAX_RING, num_sector,
                SC_MAX_SECTOR);
  EGONN_REQUIRE(n >= 0 && batch_size >= 1 && batch_size <= 65535, EGONN_ERR_INVALID,
                "scan_context: bad shape (n=%lld, batch_size=%d; batch_size in [1, 65535])", (long long)n, batch_size);
  EGONN_REQUIRE(max_length > 0.0 && max_length < 1e18 && lidar_height == lidar_height, EGONN_ERR_INVALID,
                "scan_context: max_length %g must be positive and lidar_height %g a number", max_length, lidar_height);
  EGONN_REQUIRE(scan_offsets && out_sc && (n == 0 || points), EGONN_ERR_INVALID, "scan_context: null pointer");
  ScParams P;
  P.R = num_ring;
  P.S = num_sector;
  P.gap_ring = (float)(max_length / num_ring);                 // the reference's Python floats, cast as numpy casts them
  P.gap_sector = (float)(2.0 * 3.141592653589793 / num_sector);
  P.theta_max = (float)(2.0 * 3.141592653589793 - 1e-6);
  P.lidar_height = (float)lidar_height;
  hipStream_t st = (hipStream_t)stream;
  const int cells = num_ring * num_sector;
  HIP_CHECK(hipMemsetAsync(out_sc, 0, (size_t)batch_size * cells * sizeof(float), st));
  if (n > 0) {
    int64_t G = cdiv(n, (int64_t)batch_size * SC_ROWS_PER_WG);
    G = G < 1 ? 1 : (G > SC_MAX_CHUNKS ? SC_MAX_CHUNKS : G);
    const int vec4 = ((uintptr_t)points & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(sc_cells_kernel, dim3((unsigned)G, (unsigned)batch_size), dim3(SC_WG), (size_t)cells * sizeof(uint32_t), st,
                       points, scan_offsets, n, P, vec4, reinterpret_cast<uint32_t*>(out_sc));
  }
  if (out_ringkey) {
    const int64_t rows = (int64_t)batch_size * num_ring;
    hipLaunchKernelGGL(sc_ringkey_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, st, out_sc, rows, num_sector, out_ringkey);
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_scan_context_ringkey(const float* sc, int64_t n, int num_ring, int num_sector, float* out_ringkey, void* stream) {
  EGONN_REQUIRE(sc_shape_ok(num_ring, num_sector), EGONN_ERR_INVALID,
                "scan_context_ringkey: num_ring %d outside [1, %d] or num_sector %d outside [2, %d]", num_ring, SC_MAX_RING,
                num_sector, SC_MAX_SECTOR);
  EGONN_REQUIRE(n >= 0 && n <= (1ll << 24) && (n == 0 || (sc && out_ringkey)), EGONN_ERR_INVALID,
                "scan_context_ringkey: bad arguments (n=%lld)", (long long)n);
  if (n == 0) return EGONN_OK;
  const int64_t rows = n * num_ring;
  hipLaunchKernelGGL(sc_ringkey_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, sc, rows, num_sector,
                     out_ringkey);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_scan_context_distance(const float* query_sc, int64_t n_query, const float* map_sc, int64_t n_map, int num_ring,
                                    int num_sector, const int32_t* candidates, int k, float* out_dist, int32_t* out_yaw,
                                    void* stream) {
  EGONN_REQUIRE(sc_shape_ok(num_ring, num_sector), EGONN_ERR_INVALID,
                "scan_context_distance: num_ring %d outside [1, %d] or num_sector %d outside [2, %d]", num_ring, SC_MAX_RING,
                num_sector, SC_MAX_SECTOR);
  EGONN_REQUIRE(n_query >= 0 && n_map >= 0 && n_map < (1ll << 31) && k >= 0 && (candidates || k == n_map), EGONN_ERR_INVALID,
                "scan_context_distance: bad shape (n_query=%lld, n_map=%lld, k=%d; without a candidate list k = n_map)",
                (long long)n_query, (long long)n_map, k);
  if (n_query == 0 || k == 0) return EGONN_OK;
  EGONN_REQUIRE(query_sc && out_dist && out_yaw && (n_map == 0 || map_sc), EGONN_ERR_INVALID, "scan_context_distance: null pointer");
  const size_t lds = scd_lds_bytes(num_ring, num_sector);
  static AttrOnce attr;
  if (attr.need()) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&sc_distance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)scd_lds_bytes(SC_MAX_RING, SC_MAX_SECTOR)));
    attr.mark();
  }
  // candidates per workgroup: one while the pairs are few, up to SCD_MAX_KP once there are workgroups to spare
  int64_t KP = n_query * k / 2048;
  KP = KP < 1 ? 1 : (KP > SCD_MAX_KP ? SCD_MAX_KP : KP);
  const int RS = num_ring * num_sector;
  for (int64_t q0 = 0; q0 < n_query; q0 += 65535) {
    const int64_t nq = n_query - q0 < 65535 ? n_query - q0 : 65535;
    hipLaunchKernelGGL(sc_distance_kernel, dim3((unsigned)cdiv(k, KP), (unsigned)nq), dim3(SCD_WG), lds, (hipStream_t)stream,
                       query_sc + q0 * RS, map_sc, candidates ? candidates + q0 * k : nullptr, n_map, k, num_ring, num_sector,
                       (int)KP, out_dist + q0 * k, out_yaw + q0 * k);
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_scan_context_rerank(const float* dist, const int32_t* yaw, const int32_t* candidates, int64_t n_query, int k,
                                  int32_t* out_index, float* out_dist, int32_t* out_yaw, void* stream) {
  EGONN_REQUIRE(k >= 1 && k <= SC_MAX_K, EGONN_ERR_INVALID, "scan_context_rerank: k %d outside [1, %d]", k, SC_MAX_K);
  EGONN_REQUIRE(n_query >= 0 && n_query < (1ll << 31), EGONN_ERR_INVALID, "scan_context_rerank: bad n_query %lld", (long long)n_query);
  if (n_query == 0) return EGONN_OK;
  EGONN_REQUIRE(dist && yaw && out_index && out_dist && out_yaw, EGONN_ERR_INVALID, "scan_context_rerank: null pointer");
  EGONN_REQUIRE(dist != out_dist && yaw != out_yaw && candidates != out_index, EGONN_ERR_INVALID,
                "scan_context_rerank: outputs must not alias inputs");
  hipLaunchKernelGGL(sc_rerank_kernel, dim3((unsigned)n_query), dim3(SC_MAX_K), 0, (hipStream_t)stream, dist, yaw, candidates, k,
                     out_index, out_dist, out_yaw);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
