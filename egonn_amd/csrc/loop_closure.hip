// Loop-closure detection inside one trajectory: every scan is searched against the scans that are old enough,
// a per-query window [lo, hi) of the database, and the detector is graded by its precision/recall curve.
//
// time_windows_kernel      float64 stamps -> the admissible window of every query, one binary search per bound; a second set of
//                          threads tests that the stamps are non-decreasing (status bit 0, an integer atomic).
// knn_window_kernel        egonn_knn restricted to the window, with no Q x M distance matrix: one workgroup of four waves per
//                          (query, segment of its window).  Wave w takes rows w, w + 4, ... of the segment; the distance of a row
//                          is knn_row_distance (retrieval.h), the function knn_dist_kernel calls, so the bits are egonn_knn's.
//                          Each wave keeps its k best as a sorted list, entry j in lane j: the place of a new row is the number of
//                          entries before it (ballot + popcount of the (distance, index) comparison), the entries behind it move
//                          up one lane (a shuffle).  The four lists meet in LDS and every entry finds its rank by counting.
//                          (distance, index) is a strict total order, so the k smallest are one set in one order however the rows
//                          are dealt to waves, segments or calls: ties go to the lower index, and the result of a query does not
//                          depend on the batch it is in.  +inf is a distance like any other (after the finite ones, in index
//                          order), a NaN distance is never inserted; the list ends with (-1, +inf).
//                          A batch of few queries splits every window into up to 16 segments (one workgroup each) whose lists
//                          knn_window_merge_kernel joins; the segment count depends on the number of queries only, so the scratch
//                          (n_query * segments * k pairs) does not grow with the database.
// window_radius_kernel     one wave per query: rows of the window within `radius` (recall_kernel's distance form), and the distance
//                          to the predicted row.
// pr_* kernels             scores -> monotone 32-bit keys ("no prediction" = the largest key) -> the flat radix sort of sort.hip
//                          (stable: equal scores stay in query order) -> inclusive counts by a three-launch tile scan.
#include "model.h"
#include "retrieval.h"

namespace egonn {

static constexpr int LC_BLOCK = 256;
static constexpr int LC_WAVES = LC_BLOCK / 64;
static constexpr int LC_MAX_K = 64;                 // one list entry per lane
static constexpr int LC_MAX_SEG = 16;               // segments of a window (16 * 64 list entries = 8 KiB of LDS in the merge)
static constexpr int LC_ROWS = 4;                   // rows a wave sums at a time
static constexpr int32_t LC_EMPTY = 0x7fffffff;     // index of an empty list entry (row indices stay below 2^31 - 1)

// ------------------------------------------------------------------ windows from time stamps
__global__ __launch_bounds__(LC_BLOCK) void time_windows_kernel(const double* __restrict__ t_db, int32_t m, const double* __restrict__ t_q,
                                                                int32_t nq, double min_gap, double max_gap, int32_t* __restrict__ win_lo,
                                                                int32_t* __restrict__ win_hi, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * LC_BLOCK + threadIdx.x;
  if (i < nq) {
    const double t = t_q[i], x_hi = t - min_gap, x_lo = t - max_gap;
    int32_t a = 0, b = m;                           // hi = #{j : t_db[j] <= x_hi}
    while (a < b) {
      const int32_t mid = a + ((b - a) >> 1);
      if (t_db[mid] <= x_hi) a = mid + 1; else b = mid;
    }
    win_hi[i] = a;
    a = 0, b = m;                                   // lo = #{j : t_db[j] < x_lo}
    while (a < b) {
      const int32_t mid = a + ((b - a) >> 1);
      if (t_db[mid] < x_lo) a = mid + 1; else b = mid;
    }
    win_lo[i] = a;
  }
  if (i + 1 < m && !(t_db[i] <= t_db[i + 1])) atomicOr(status, 1);      // a NaN stamp is out of order too
}

API int egonn_time_windows(const double* t_db, int64_t m, const double* t_q, int64_t n_query, double min_gap, double max_gap,
                           int32_t* win_lo, int32_t* win_hi, int32_t* status, void* stream) {
  EGONN_REQUIRE(m >= 0 && m < (1ll << 31) && n_query >= 0 && n_query < (1ll << 31), EGONN_ERR_INVALID,
                "time_windows: m=%lld n_query=%lld outside [0, 2^31)", (long long)m, (long long)n_query);
  EGONN_REQUIRE(status && (m == 0 || t_db) && (n_query == 0 || (t_q && win_lo && win_hi)), EGONN_ERR_INVALID,
                "time_windows: null pointer");
  EGONN_REQUIRE(min_gap == min_gap && max_gap == max_gap, EGONN_ERR_INVALID, "time_windows: a gap is NaN");
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  const int64_t threads = n_query > m - 1 ? n_query : m - 1;
  if (threads <= 0) return EGONN_OK;
  hipLaunchKernelGGL(time_windows_kernel, dim3((unsigned)cdiv(threads, LC_BLOCK)), dim3(LC_BLOCK), 0, st, t_db, (int32_t)m, t_q,
                     (int32_t)n_query, min_gap, max_gap, win_lo, win_hi, status);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ windowed kNN
__device__ static inline bool knn_before(float av, int32_t ai, float bv, int32_t bi) { return av < bv || (av == bv && ai < bi); }

// one wave's sorted list (entry j in lane j, lanes >= k unused): take (v, r) in if it belongs to the k best
__device__ static inline void knn_list_insert(float& lv, int32_t& li, float v, int32_t r, int k, int lane) {
  if (v != v) return;                                                   // wave-uniform: v is the same in every lane
  const uint64_t kmask = k >= 64 ? ~0ull : ((1ull << k) - 1);
  const int pos = __popcll(__ballot(knn_before(lv, li, v, r)) & kmask);   // sorted: the entries before (v, r) are a prefix
  if (pos >= k) return;
  const float uv = __shfl_up(lv, 1, 64);
  const int32_t ui = __shfl_up(li, 1, 64);
  if (lane == pos) {
    lv = v;
    li = r;
  } else if (lane > pos) {
    lv = uv;
    li = ui;
  }
}

// n list entries in LDS (LC_EMPTY = none) -> the k best in order at out_idx / out_dist, (-1, +inf) behind them.  The whole
// workgroup calls it after a barrier that made the entries and *s_valid = 0 visible.
__device__ static inline void knn_merge_emit(const float* s_v, const int32_t* s_i, int n, int k, int32_t* s_valid,
                                             int32_t* __restrict__ out_idx, float* __restrict__ out_dist) {
  const int t = threadIdx.x;
  int valid = 0;
  for (int e = t; e < n; e += LC_BLOCK) {
    const float v = s_v[e];
    const int32_t i = s_i[e];
    if (i == LC_EMPTY) continue;
    ++valid;
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += knn_before(s_v[j], s_i[j], v, i) ? 1 : 0;
    if (rank < k) {
      out_idx[rank] = i;
      out_dist[rank] = v;
    }
  }
  if (valid) atomicAdd(s_valid, valid);
  __syncthreads();
  for (int p = t; p < k; p += LC_BLOCK)
    if (p >= *s_valid) {
      out_idx[p] = -1;
      out_dist[p] = INFINITY;
    }
}

// grid (n_query, nseg); dst: (n_query, nseg, k)
__global__ __launch_bounds__(LC_BLOCK) void knn_window_kernel(const float* __restrict__ query, const float* __restrict__ db, int32_t m,
                                                              int d, int k, const int32_t* __restrict__ win_lo,
                                                              const int32_t* __restrict__ win_hi, int32_t* __restrict__ dst_idx,
                                                              float* __restrict__ dst_dist) {
  extern __shared__ float s_q[];
  __shared__ float s_v[LC_WAVES * LC_MAX_K];
  __shared__ int32_t s_i[LC_WAVES * LC_MAX_K];
  __shared__ int32_t s_valid;
  const int q = blockIdx.x, seg = blockIdx.y, nseg = gridDim.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int i = t; i < d; i += LC_BLOCK) s_q[i] = query[(int64_t)q * d + i];
  if (t == 0) s_valid = 0;
  __syncthreads();
  int32_t lo = win_lo ? win_lo[q] : 0, hi = win_hi[q];
  lo = lo < 0 ? 0 : lo;
  hi = hi > m ? m : hi;
  const int64_t len = hi > lo ? hi - lo : 0, chunk = (len + nseg - 1) / nseg;
  const int64_t a64 = (int64_t)seg * chunk, b64 = a64 + chunk;
  const int32_t a = lo + (int32_t)(a64 < len ? a64 : len), b = lo + (int32_t)(b64 < len ? b64 : len);

  float lv = INFINITY;
  int32_t li = LC_EMPTY;
  const int64_t step = (int64_t)LC_WAVES * d;
  int64_t r = (int64_t)a + w;                         // 64-bit: r + 12 may pass 2^31
  for (; r + LC_WAVES * (LC_ROWS - 1) < b; r += LC_WAVES * LC_ROWS) {
    float v[LC_ROWS];
    knn_row_distance<LC_ROWS>(db + r * d, step, s_q, d, lane, v);
#pragma unroll
    for (int u = 0; u < LC_ROWS; ++u) knn_list_insert(lv, li, __shfl(v[u], 0, 64), (int32_t)(r + LC_WAVES * u), k, lane);
  }
  for (; r < b; r += LC_WAVES) {
    float v[1];
    knn_row_distance<1>(db + r * d, 0, s_q, d, lane, v);
    knn_list_insert(lv, li, __shfl(v[0], 0, 64), (int32_t)r, k, lane);
  }
  if (lane < k) {
    s_v[w * k + lane] = lv;
    s_i[w * k + lane] = li;
  }
  __syncthreads();
  const int64_t o = ((int64_t)q * nseg + seg) * k;
  knn_merge_emit(s_v, s_i, LC_WAVES * k, k, &s_valid, dst_idx + o, dst_dist + o);
}

// part_*: (n_query, nseg, k) lists as knn_window_kernel writes them -> out (n_query, k)
__global__ __launch_bounds__(LC_BLOCK) void knn_window_merge_kernel(const int32_t* __restrict__ part_idx, const float* __restrict__ part_dist,
                                                                    int nseg, int k, int32_t* __restrict__ out_idx,
                                                                    float* __restrict__ out_dist) {
  __shared__ float s_v[LC_MAX_SEG * LC_MAX_K];
  __shared__ int32_t s_i[LC_MAX_SEG * LC_MAX_K];
  __shared__ int32_t s_valid;
  const int q = blockIdx.x, t = threadIdx.x, n = nseg * k;
  for (int e = t; e < n; e += LC_BLOCK) {
    const int32_t i = part_idx[(int64_t)q * n + e];
    s_v[e] = part_dist[(int64_t)q * n + e];
    s_i[e] = i < 0 ? LC_EMPTY : i;
  }
  if (t == 0) s_valid = 0;
  __syncthreads();
  knn_merge_emit(s_v, s_i, n, k, &s_valid, out_idx + (int64_t)q * k, out_dist + (int64_t)q * k);
}

// segments per window: enough workgroups for a batch of few queries, one for a batch that fills the device by itself
static int knn_window_segments(int64_t nq) {
  if (nq <= 0 || nq >= 512) return 1;
  const int64_t s = cdiv(1024, nq);
  return (int)(s > LC_MAX_SEG ? LC_MAX_SEG : s);
}

static bool knn_window_sizes_ok(int64_t nq, int k) { return nq >= 0 && nq < (1ll << 31) && k >= 1 && k <= LC_MAX_K; }

API int64_t egonn_knn_window_scratch_bytes(int64_t n_query, int k) {
  if (!knn_window_sizes_ok(n_query, k)) return -1;
  const int nseg = knn_window_segments(n_query);
  return nseg == 1 ? 0 : n_query * nseg * k * 8;
}

API int egonn_knn_window(const float* query, int64_t n_query, const float* db, int64_t n_database, int d, int k, const int32_t* win_lo,
                         const int32_t* win_hi, int32_t* out_idx, float* out_dist, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(knn_window_sizes_ok(n_query, k) && n_database >= 0 && n_database < (1ll << 31) && d >= 1 && d <= 4096,
                EGONN_ERR_INVALID, "knn_window: bad arguments (n_query=%lld n_database=%lld d=%d k=%d; 1 <= k <= %d, 1 <= d <= 4096)",
                (long long)n_query, (long long)n_database, d, k, LC_MAX_K);
  if (n_query == 0) return EGONN_OK;
  EGONN_REQUIRE(query && win_hi && out_idx && out_dist && (db || n_database == 0), EGONN_ERR_INVALID, "knn_window: null pointer");
  const int nseg = knn_window_segments(n_query);
  const int64_t need = egonn_knn_window_scratch_bytes(n_query, k);
  EGONN_REQUIRE(need == 0 || (scratch && scratch_bytes >= need && ((uintptr_t)scratch & 7) == 0), EGONN_ERR_INVALID,
                "knn_window: scratch needs %lld bytes, 8-byte aligned", (long long)need);
  hipStream_t st = (hipStream_t)stream;
  const int32_t m = (int32_t)n_database;
  int32_t* part_idx = nseg == 1 ? out_idx : (int32_t*)scratch;
  float* part_dist = nseg == 1 ? out_dist : (float*)scratch + n_query * nseg * k;
  hipLaunchKernelGGL(knn_window_kernel, dim3((unsigned)n_query, (unsigned)nseg), dim3(LC_BLOCK), (size_t)d * 4, st, query, db, m, d, k,
                     win_lo, win_hi, part_idx, part_dist);
  if (nseg > 1)
    hipLaunchKernelGGL(knn_window_merge_kernel, dim3((unsigned)n_query), dim3(LC_BLOCK), 0, st, part_idx, part_dist, nseg, k, out_idx,
                       out_dist);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ true revisits inside the window
__global__ __launch_bounds__(LC_BLOCK) void window_radius_kernel(const float* __restrict__ qpos, int32_t nq, const float* __restrict__ dbpos,
                                                                 int32_t m, int pd, const int32_t* __restrict__ win_lo,
                                                                 const int32_t* __restrict__ win_hi, float radius,
                                                                 const int32_t* __restrict__ pred, int32_t* __restrict__ count,
                                                                 float* __restrict__ pred_dist) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * LC_WAVES + (threadIdx.x >> 6);
  if (q >= nq) return;                               // wave-uniform
  float p[3] = {0.f, 0.f, 0.f};
  for (int c = 0; c < pd; ++c) p[c] = qpos[q * pd + c];
  int32_t lo = win_lo ? win_lo[q] : 0, hi = win_hi[q];
  lo = lo < 0 ? 0 : lo;
  hi = hi > m ? m : hi;
  int32_t n = 0;
  for (int64_t j = (int64_t)lo + lane; j < hi; j += 64) {
    float s = 0.f;
    for (int c = 0; c < pd; ++c) {
      const float df = p[c] - dbpos[j * pd + c];
      s = fmaf(df, df, s);
    }
    n += sqrtf(s) <= radius ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (lane == 0) {
    count[q] = n;
    if (pred) {
      const int32_t j = pred[q];
      float dist = INFINITY;
      if (j >= 0 && j < m) {
        float s = 0.f;
        for (int c = 0; c < pd; ++c) {
          const float df = p[c] - dbpos[(int64_t)j * pd + c];
          s = fmaf(df, df, s);
        }
        dist = sqrtf(s);
      }
      pred_dist[q] = dist;
    }
  }
}

API int egonn_window_radius(const float* qpos, int64_t n_query, const float* dbpos, int64_t m, int pd, const int32_t* win_lo,
                            const int32_t* win_hi, float radius, const int32_t* pred, int32_t* count, float* pred_dist, void* stream) {
  EGONN_REQUIRE(n_query >= 0 && n_query < (1ll << 31) && m >= 0 && m < (1ll << 31) && (pd == 2 || pd == 3), EGONN_ERR_INVALID,
                "window_radius: bad arguments (n_query=%lld m=%lld pd=%d; pd is 2 or 3)", (long long)n_query, (long long)m, pd);
  if (n_query == 0) return EGONN_OK;
  EGONN_REQUIRE(qpos && win_hi && count && (dbpos || m == 0) && (!pred || pred_dist), EGONN_ERR_INVALID, "window_radius: null pointer");
  hipLaunchKernelGGL(window_radius_kernel, dim3((unsigned)cdiv(n_query, LC_WAVES)), dim3(LC_BLOCK), 0, (hipStream_t)stream, qpos,
                     (int32_t)n_query, dbpos, (int32_t)m, pd, win_lo, win_hi, radius, pred, count, pred_dist);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ precision/recall curve
static constexpr int PR_ITEMS = 4;                            // consecutive positions per thread
static constexpr int PR_TILE = LC_BLOCK * PR_ITEMS;
static constexpr uint64_t PR_NONE = 0xffffffffull;            // key of "no prediction": behind every score

// ascending float order as ascending unsigned order; -0.0 is +0.0; +inf and NaN are no prediction
__device__ static inline uint64_t pr_key(float s) {
  if (s != s || s == INFINITY) return PR_NONE;
  const uint32_t u = s == 0.f ? 0u : __float_as_uint(s);
  return (u & 0x80000000u) ? (uint32_t)~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(LC_BLOCK) void pr_key_kernel(const float* __restrict__ score, const int32_t* __restrict__ revisit, int32_t n,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          int32_t* __restrict__ totals) {
  const int64_t i = (int64_t)blockIdx.x * LC_BLOCK + threadIdx.x;
  bool predicted = false, rev = false;
  if (i < n) {
    const uint64_t key = pr_key(score[i]);
    keys[i] = key;
    vals[i] = (uint32_t)i;
    predicted = key != PR_NONE;
    rev = revisit[i] != 0;
  }
  const uint64_t mp = __ballot(predicted), mr = __ballot(rev);
  if ((threadIdx.x & 63) == 0) {
    if (mp) atomicAdd(&totals[0], (int32_t)__popcll(mp));
    if (mr) atomicAdd(&totals[1], (int32_t)__popcll(mr));
  }
}

// exclusive prefix of x over the workgroup's threads; *total: the workgroup's sum.  s_w: LC_WAVES ints of LDS.
__device__ static inline int32_t pr_block_scan(int32_t x, int32_t* s_w, int32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  __syncthreads();                                   // s_w may still be read from the call before
  if (lane == 63) s_w[w] = incl;
  __syncthreads();
  int32_t base = 0, sum = 0;
#pragma unroll
  for (int j = 0; j < LC_WAVES; ++j) {
    if (j < w) base += s_w[j];
    sum += s_w[j];
  }
  *total = sum;
  return base + incl - x;
}

// the three flags of sorted position p: bit 0 true positive, bit 1 false positive, bit 2 revisit (0 beyond the predictions)
__device__ static inline int pr_flags(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                      const int32_t* __restrict__ correct, const int32_t* __restrict__ revisit, int64_t p, int32_t n) {
  if (p >= n || keys[p] == PR_NONE) return 0;
  const uint32_t i = vals[p];
  return (correct[i] != 0 ? 1 : 2) | (revisit[i] != 0 ? 4 : 0);
}

// sums (3, tiles): the flag counts of every tile
__global__ __launch_bounds__(LC_BLOCK) void pr_tile_sums_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                const int32_t* __restrict__ correct, const int32_t* __restrict__ revisit,
                                                                int32_t n, int32_t tiles, int32_t* __restrict__ sums) {
  __shared__ int32_t s_w[LC_WAVES];
  int32_t c[3] = {0, 0, 0};
  const int64_t p0 = ((int64_t)blockIdx.x * LC_BLOCK + threadIdx.x) * PR_ITEMS;
  for (int u = 0; u < PR_ITEMS; ++u) {
    const int f = pr_flags(keys, vals, correct, revisit, p0 + u, n);
    c[0] += f & 1, c[1] += (f >> 1) & 1, c[2] += (f >> 2) & 1;
  }
  for (int j = 0; j < 3; ++j) {
    int32_t total;
    (void)pr_block_scan(c[j], s_w, &total);
    if (threadIdx.x == 0) sums[(int64_t)j * tiles + blockIdx.x] = total;
  }
}

// one workgroup: sums (3, tiles) -> their exclusive prefixes, in place
__global__ __launch_bounds__(LC_BLOCK) void pr_scan_sums_kernel(int32_t tiles, int32_t* __restrict__ sums) {
  __shared__ int32_t s_w[LC_WAVES];
  for (int j = 0; j < 3; ++j) {
    int32_t carry = 0;
    for (int32_t b0 = 0; b0 < tiles; b0 += LC_BLOCK) {
      const int32_t b = b0 + threadIdx.x;
      const int32_t x = b < tiles ? sums[(int64_t)j * tiles + b] : 0;
      int32_t total;
      const int32_t ex = pr_block_scan(x, s_w, &total);
      if (b < tiles) sums[(int64_t)j * tiles + b] = carry + ex;
      carry += total;
    }
  }
}

__global__ __launch_bounds__(LC_BLOCK) void pr_emit_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                           const int32_t* __restrict__ correct, const int32_t* __restrict__ revisit, int32_t n,
                                                           int32_t tiles, const int32_t* __restrict__ sums, int32_t* __restrict__ order,
                                                           int32_t* __restrict__ cum_tp, int32_t* __restrict__ cum_fp,
                                                           int32_t* __restrict__ cum_rev, uint8_t* __restrict__ group_end) {
  __shared__ int32_t s_w[LC_WAVES];
  int f[PR_ITEMS];
  int32_t c[3] = {0, 0, 0};
  const int64_t p0 = ((int64_t)blockIdx.x * LC_BLOCK + threadIdx.x) * PR_ITEMS;
  for (int u = 0; u < PR_ITEMS; ++u) {
    f[u] = pr_flags(keys, vals, correct, revisit, p0 + u, n);
    c[0] += f[u] & 1, c[1] += (f[u] >> 1) & 1, c[2] += (f[u] >> 2) & 1;
  }
  int32_t run[3];
  for (int j = 0; j < 3; ++j) {
    int32_t total;
    run[j] = sums[(int64_t)j * tiles + blockIdx.x] + pr_block_scan(c[j], s_w, &total);
  }
  for (int u = 0; u < PR_ITEMS; ++u) {
    const int64_t p = p0 + u;
    if (p >= n) break;
    run[0] += f[u] & 1, run[1] += (f[u] >> 1) & 1, run[2] += (f[u] >> 2) & 1;
    const uint64_t key = keys[p];
    order[p] = (int32_t)vals[p];
    cum_tp[p] = run[0];
    cum_fp[p] = run[1];
    cum_rev[p] = run[2];
    group_end[p] = key != PR_NONE && (p + 1 == n || keys[p + 1] != key) ? 1 : 0;
  }
}

// the carves of the PR curve's scratch span.  With scratch = nullptr only `total` means anything
struct PrSpan {
  uint64_t* keys[2];        // ping-pong buffers of the sort
  uint32_t* vals[2];
  int32_t* sums;
  Arena sort_ws;
  size_t total;
};
static PrSpan pr_span(void* scratch, int64_t n) {
  PrSpan S;
  Carve c(scratch);
  const size_t nn = (size_t)(n > 0 ? n : 1), tiles = (size_t)cdiv((int64_t)nn, PR_TILE);
  for (int k = 0; k < 2; ++k) S.keys[k] = c.take<uint64_t>(nn);
  for (int k = 0; k < 2; ++k) S.vals[k] = c.take<uint32_t>(nn);
  S.sums = c.take<int32_t>(3 * tiles);
  S.sort_ws = c.sort_arena(radix_sort_scratch_bytes(n));
  S.total = c.total();
  return S;
}

API int64_t egonn_pr_curve_scratch_bytes(int64_t n) {
  if (n < 0 || n >= (1ll << 31)) return -1;
  return (int64_t)pr_span(nullptr, n).total;
}

API int egonn_pr_curve(const float* score, const int32_t* correct, const int32_t* revisit, int64_t n, int32_t* order, int32_t* cum_tp,
                       int32_t* cum_fp, int32_t* cum_rev, uint8_t* group_end, int32_t* totals, void* scratch, int64_t scratch_bytes,
                       void* stream) {
  EGONN_REQUIRE(n >= 0 && n < (1ll << 31), EGONN_ERR_INVALID, "pr_curve: n=%lld outside [0, 2^31)", (long long)n);
  EGONN_REQUIRE(totals && (n == 0 || (score && correct && revisit && order && cum_tp && cum_fp && cum_rev && group_end)),
                EGONN_ERR_INVALID, "pr_curve: null pointer");
  PrSpan S = pr_span(scratch, n);
  if (n > 0) EGONN_TRY(span_check("pr_curve", scratch, scratch_bytes, S.total));      // no row: no scratch, null is fine
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(totals, 0, 2 * sizeof(int32_t), st));
  if (n == 0) return EGONN_OK;
  uint64_t *keys0 = S.keys[0], *keys1 = S.keys[1];
  uint32_t *vals0 = S.vals[0], *vals1 = S.vals[1];
  int32_t* sums = S.sums;
  const int32_t nn = (int32_t)n, tiles = (int32_t)cdiv(n, PR_TILE);
  hipLaunchKernelGGL(pr_key_kernel, dim3((unsigned)cdiv(n, LC_BLOCK)), dim3(LC_BLOCK), 0, st, score, revisit, nn, keys0, vals0, totals);
  uint64_t* kres = keys1;
  uint32_t* vres = vals1;
  EGONN_TRY(radix_sort_pairs(S.sort_ws, keys0, vals0, keys1, vals1, n, 32, st, nullptr, &kres, &vres));
  hipLaunchKernelGGL(pr_tile_sums_kernel, dim3((unsigned)tiles), dim3(LC_BLOCK), 0, st, kres, vres, correct, revisit, nn, tiles, sums);
  hipLaunchKernelGGL(pr_scan_sums_kernel, dim3(1), dim3(LC_BLOCK), 0, st, tiles, sums);
  hipLaunchKernelGGL(pr_emit_kernel, dim3((unsigned)tiles), dim3(LC_BLOCK), 0, st, kres, vres, correct, revisit, nn, tiles, sums, order,
                     cum_tp, cum_fp, cum_rev, group_end);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn
