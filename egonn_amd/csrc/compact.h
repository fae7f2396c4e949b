// Workgroup compaction, stated once for voxel_map.hip, voxel_key.h, icp.hip (the downsample) and ndt.hip: flag rows, count the
// flags per workgroup (wg_count), scan the counts in one workgroup (wg_scan), give every flagged row its output slot (wg_rank);
// and the bounds of a run of equal rows inside a wave (wave_run).  Device only.  WG is the workgroup size, a multiple of 64;
// every thread of the workgroup calls (the functions hold barriers).  Each function owns its LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace egonn {

// the sum over the workgroup of one value per wave (lane 0's): to every thread.  Begins with the barrier that keeps a second
// call in the same kernel (a loop) from overwriting sums that a slower wave has not read yet
template <int WG>
__device__ __forceinline__ int wg_wave_sum(int wave_value) {
  static_assert(WG % 64 == 0 && WG >= 64 && WG <= 1024, "whole waves");
  __shared__ int s_w[WG / 64];
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = wave_value;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int k = 0; k < WG / 64; ++k) total += s_w[k];
  return total;
}

// flagged threads of the workgroup: to every thread
template <int WG>
__device__ __forceinline__ int wg_count(bool flag) {
  return wg_wave_sum<WG>(__popcll(__ballot(flag)));
}

// flagged threads in front of this one, from bal = __ballot(flag) (the caller keeps the ballot: wave_run reads it too), and the
// workgroup's count in *total when asked for.  Like wg_wave_sum it begins with the barrier that protects its LDS from the
// previous call, so a kernel may call it once per tile of a loop whose trip count is uniform
template <int WG>
__device__ __forceinline__ int wg_rank(unsigned long long bal, int* total = nullptr) {
  static_assert(WG % 64 == 0 && WG >= 64 && WG <= 1024, "whole waves");
  __shared__ int s_w[WG / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s_w[w] = __popcll(bal);
  __syncthreads();
  int r = __popcll(bal & ((1ull << lane) - 1ull)), sum = 0;
#pragma unroll
  for (int k = 0; k < WG / 64; ++k) {
    if (k < w) r += s_w[k];
    sum += s_w[k];
  }
  if (total) *total = sum;
  return r;
}

// one workgroup: the exclusive scan of n counters, get(b) -> put(b, sum of get(0 .. b), total); the total to every thread.
// Thread t owns the ceil(n / WG) consecutive counters from t * ceil(n / WG) on and reads each of them twice; sums are 64-bit
template <int WG, class Get, class Put>
__device__ __forceinline__ int64_t wg_scan(int64_t n, Get get, Put put) {
  __shared__ int64_t s_sum[WG + 1];
  const int t = threadIdx.x;
  const int64_t per = (n + WG - 1) / WG;
  const int64_t b0 = t * per < n ? t * per : n, b1 = b0 + per < n ? b0 + per : n;
  int64_t s = 0;
  for (int64_t b = b0; b < b1; ++b) s += get(b);
  s_sum[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t acc = 0;
    for (int k = 0; k < WG; ++k) {
      const int64_t v = s_sum[k];
      s_sum[k] = acc;
      acc += v;
    }
    s_sum[WG] = acc;
  }
  __syncthreads();
  const int64_t total = s_sum[WG];
  int64_t acc = s_sum[t];
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t v = get(b);
    put(b, acc, total);
    acc += v;
  }
  return total;
}
// the same over an array, in place
template <int WG>
__device__ __forceinline__ int64_t wg_scan(int32_t* __restrict__ cnt, int64_t n) {
  return wg_scan<WG>(n, [&](int64_t b) { return (int64_t)cnt[b]; }, [&](int64_t b, int64_t pre, int64_t) { cnt[b] = (int32_t)pre; });
}

// Runs of equal rows in consecutive lanes, from the ballot of their heads: the lanes up to this one, the first lane of this
// lane's run inside the wave (lane 0 for a run that came in from the wave before) and whether the run begins in this wave.  A
// segmented scan adds the value from d lanes below while lane - d >= start; the callers keep their ladders
struct WaveRun {
  unsigned long long upto;
  int start;
  bool begins_here;
};
__device__ __forceinline__ WaveRun wave_run(unsigned long long heads) {
  const int lane = threadIdx.x & 63;
  WaveRun r;
  r.upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  const unsigned long long hb = heads & r.upto;
  r.start = hb ? 63 - __clzll((long long)hb) : 0;
  r.begins_here = (heads >> r.start) & 1ull;
  return r;
}

}  // namespace egonn
