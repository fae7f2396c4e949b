// Place-recognition retrieval on the device — the step right after the descriptor path in the database build
// (BASELINE configs[4]; reference eval/evaluate.py:60-88 and :168-184):
//     embed_dist = np.linalg.norm(map_embeddings - query_embedding, axis=1);  nn_ndx = np.argsort(embed_dist)[:k]
//     euclid_dist = norm(query_pos - map_positions[nn_ndx]);  tp[r][nn] += any(euclid_dist[:nn+1] <= r)
// knn_dist_kernel: one workgroup per query, one wave per database row at a time, exact difference form (not the
// |a|^2+|b|^2-2ab expansion) like the reference; the row distance is knn_row_distance (retrieval.h), shared with the
// windowed search of loop_closure.hip, whose distances are these bit for bit.
// knn_select_kernel: k rounds of a workgroup-wide arg-min over the query's distance row (ties: lower index).
// Non-finite distances: +inf (an overflowing or infinite element) is a distance like any other, after every finite one
// and in index order; a NaN distance is never a neighbour, the list then ends early with (-1, +inf).  A taken entry is
// marked NaN, which no comparison selects, so that a genuine +inf is returned once and only once.
#include "model.h"
#include "retrieval.h"

namespace egonn {

__global__ __launch_bounds__(256) void knn_dist_kernel(const float* __restrict__ query, const float* __restrict__ db,
                                                      int32_t m, int d, float* __restrict__ dist) {
  extern __shared__ float s_q[];
  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int i = t; i < d; i += 256) s_q[i] = query[(int64_t)q * d + i];
  __syncthreads();
  for (int32_t r = w; r < m; r += 4) {
    float v[1];
    knn_row_distance<1>(db + (int64_t)r * d, 0, s_q, d, lane, v);
    if (lane == 0) dist[(int64_t)q * m + r] = v[0];
  }
}

__global__ __launch_bounds__(256) void knn_select_kernel(float* __restrict__ dist, int32_t m, int k,
                                                        int32_t* __restrict__ out_idx, float* __restrict__ out_dist) {
  __shared__ float s_v[4];
  __shared__ int32_t s_i[4];
  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  float* row = dist + (int64_t)q * m;
  for (int round = 0; round < k; ++round) {
    float bv = INFINITY;
    int32_t bi = 0x7fffffff;
    for (int32_t i = t; i < m; i += 256) {
      const float v = row[i];
      if (v < bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int32_t oi = __shfl_xor(bi, o, 64);
      if (ov < bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      s_v[w] = bv;
      s_i[w] = bi;
    }
    __syncthreads();
    if (t == 0) {
      for (int j = 1; j < 4; ++j)
        if (s_v[j] < s_v[0] || (s_v[j] == s_v[0] && s_i[j] < s_i[0])) {
          s_v[0] = s_v[j];
          s_i[0] = s_i[j];
        }
      const bool ok = s_i[0] != 0x7fffffff;       // nothing left to take: every entry taken (round >= m) or NaN
      out_idx[(int64_t)q * k + round] = ok ? s_i[0] : -1;
      out_dist[(int64_t)q * k + round] = ok ? s_v[0] : INFINITY;
      if (ok) row[s_i[0]] = NAN;                  // taken: never compares below or equal to anything
    }
    __syncthreads();
  }
}

API int egonn_knn(const float* query, int64_t n_query, const float* db, int64_t n_database, int d, int k, int32_t* out_idx,
                  float* out_dist, float* scratch, int64_t scratch_floats, void* stream) {
  EGONN_REQUIRE(n_query < (1ll << 31) && n_database < (1ll << 31), EGONN_ERR_INVALID, "knn: too many rows");
  const int32_t nq = (int32_t)n_query, m = (int32_t)n_database;
  EGONN_REQUIRE(query && db && out_idx && out_dist && nq >= 0 && m >= 1 && d >= 1 && d <= 4096 && k >= 1, EGONN_ERR_INVALID,
                "knn: bad arguments (nq=%d m=%d d=%d k=%d)", nq, m, d, k);
  if (nq == 0) return EGONN_OK;
  EGONN_REQUIRE(scratch && (size_t)scratch_floats >= (size_t)nq * m, EGONN_ERR_INVALID,
                "knn: scratch needs %lld floats", (long long)nq * m);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(knn_dist_kernel, dim3((unsigned)nq), dim3(256), (size_t)d * 4, st, query, db, m, d, scratch);
  hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)nq), dim3(256), 0, st, scratch, m, k, out_idx, out_dist);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// tp[r][nn] = number of queries with a retrieved neighbour among the first nn+1 whose position lies within radius[r]
__global__ void recall_kernel(const int32_t* __restrict__ nn_idx, const float* __restrict__ qpos,
                              const float* __restrict__ mpos, int32_t nq, int k, int pd, const float* __restrict__ radius,
                              int nr, int32_t* __restrict__ tp) {
  const int32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  float best = INFINITY;
  for (int nn = 0; nn < k; ++nn) {
    const int32_t j = nn_idx[(int64_t)q * k + nn];
    if (j >= 0) {
      float s = 0.f;
      for (int c = 0; c < pd; ++c) {
        const float df = qpos[(int64_t)q * pd + c] - mpos[(int64_t)j * pd + c];
        s = fmaf(df, df, s);
      }
      best = fminf(best, sqrtf(s));
    }
    for (int r = 0; r < nr; ++r)
      if (best <= radius[r]) atomicAdd(&tp[r * k + nn], 1);
  }
}

API int egonn_recall_counts(const int32_t* nn_idx, const float* qpos, const float* mpos, int64_t n_query, int k, int pd,
                            const float* radius, int nr, int32_t* tp, void* stream) {
  const int32_t nq = (int32_t)n_query;
  hipStream_t st = (hipStream_t)stream;
  EGONN_REQUIRE(radius && tp && k >= 1 && nr >= 1 && pd >= 1 && nq >= 0 && (nq == 0 || (nn_idx && qpos && mpos)),
                EGONN_ERR_INVALID, "recall: bad arguments");       // an empty query set has no buffers to point at
  HIP_CHECK(hipMemsetAsync(tp, 0, (size_t)nr * k * 4, st));
  if (nq == 0) return EGONN_OK;
  hipLaunchKernelGGL(recall_kernel, dim3((unsigned)cdiv(nq, 128)), dim3(128), 0, st, nn_idx, qpos, mpos, nq, k, pd,
                     radius, nr, tp);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn
