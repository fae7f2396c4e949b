// The point arithmetic of the voxel map, stated once for voxel_map.hip and ndt.hip (include/egonn_hip.h, "voxel map"): the
// frame, the 63-bit key and the residuals of a posed point, the picked clouds of a call and their offsets, the search in a
// sorted key array.  Every floating-point operation is the IEEE operation that is written (contraction off).
#pragma once
#include "../../include/egonn_hip.h"
#include "common.h"
#include "compact.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int VM_WG = 256;
static constexpr int VM_BITS = 21;                       // index bits per axis
static constexpr int64_t VM_BIAS = 1ll << 20;
static constexpr int64_t VM_ONE = 1ll << 30;             // fixed-point one of a residual
static constexpr uint64_t VM_MASK = (1ull << VM_BITS) - 1ull;
static constexpr uint64_t VM_INVALID = ~0ull;            // key of a dropped point (valid keys have bit 63 clear): sorts last
static constexpr int VM_MAX_OBS = 4096;

struct VmFrame { double org[3]; double voxel; };

__device__ static inline int64_t vm_live(const int64_t* __restrict__ n_dev, int64_t cap) { return clipi(*n_dev, cap); }

// first position in [0, n) whose key is >= k
__device__ static inline int64_t vm_lower_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ static inline uint64_t vm_pack_key(const uint64_t* idx) { return (idx[0] << (2 * VM_BITS)) | (idx[1] << VM_BITS) | idx[2]; }

// point p (3) of an observation under the pose X (4 x 4, row-major) in frame F: false for a dropped point (an index outside 21
// bits, a non-finite coordinate), else its key and its residuals r (3) in 2^-30 voxel units
__device__ static inline bool vm_point_key(const double* __restrict__ p, const double* __restrict__ X, const VmFrame& F, uint64_t* key,
                                           int* r) {
  const double p0 = p[0], p1 = p[1], p2 = p[2];
  uint64_t idx[3];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double tt = X[a * 4 + 3] - F.org[a];
    const double w = ((X[a * 4] * p0 + X[a * 4 + 1] * p1) + X[a * 4 + 2] * p2) + tt;
    const double s = w / F.voxel;
    const double f = floor(s);
    ok = ok && f >= -(double)VM_BIAS && f < (double)VM_BIAS;             // false for NaN / inf as well
    const int64_t qa = ok ? (int64_t)floor((s - f) * (double)VM_ONE) : 0;
    idx[a] = ok ? (uint64_t)((int64_t)f + VM_BIAS) : 0ull;
    r[a] = (int)(qa < VM_ONE - 1 ? qa : VM_ONE - 1);
  }
  if (ok) *key = vm_pack_key(idx);
  return ok;
}

// picked cloud of observation k: [lo, hi) in the bank, empty for a pick outside it
__device__ static inline bool vm_pick_range(const int64_t* __restrict__ off, int64_t n_bank, int64_t n_clouds, int32_t p, int64_t* lo,
                                            int64_t* hi) {
  *lo = *hi = 0;
  if (p < 0 || (int64_t)p >= n_clouds) return false;
  const int64_t a = clipi(off[p], n_bank), b = clipi(off[p + 1], n_bank);
  *lo = a;
  *hi = b > a ? b : a;
  return true;
}

// one workgroup: obs_off (n_obs + 1) = the scan of the picked clouds' sizes; BAD_INDEX for a pick outside the bank; more points
// than points_capacity: CAPACITY and every offset zero
__global__ __launch_bounds__(VM_WG) static void vm_offsets_kernel(const int64_t* __restrict__ off, int64_t n_bank, int64_t n_clouds,
                                                                  const int32_t* __restrict__ pick, int n_obs, int64_t points_capacity,
                                                                  int64_t* __restrict__ obs_off, int32_t* __restrict__ status) {
  bool bad = false;
  auto size = [&](int64_t k) {
    int64_t lo, hi;
    bad = !vm_pick_range(off, n_bank, n_clouds, pick[k], &lo, &hi) || bad;
    return hi - lo;
  };
  // more points than the caller made room for: no point at all
  const int64_t total = wg_scan<VM_WG>(n_obs, size, [&](int64_t k, int64_t before, int64_t all) {
    obs_off[k] = all > points_capacity ? 0 : before;
  });
  if (bad) atomicOr(status, EGONN_VMAP_STATUS_BAD_INDEX);
  if (threadIdx.x == 0) {
    if (total > points_capacity) atomicOr(status, EGONN_VMAP_STATUS_CAPACITY);
    obs_off[n_obs] = total > points_capacity ? 0 : total;
  }
}

// point i of a call: the last observation k with obs_off[k] <= i (its cloud is not empty, i < total) and the bank row, -1 when
// the row lies outside the picked cloud
__device__ static inline int vm_point_source(const int64_t* __restrict__ obs_off, int n_obs, const int64_t* __restrict__ off,
                                             int64_t n_bank, int64_t n_clouds, const int32_t* __restrict__ pick, int64_t i,
                                             int64_t* src) {
  int lo = 0, hi = n_obs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (obs_off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  int64_t c0, c1;
  vm_pick_range(off, n_bank, n_clouds, pick[lo], &c0, &c1);
  const int64_t s = c0 + (i - obs_off[lo]);
  *src = s >= c0 && s < c1 ? s : -1;
  return lo;
}

static inline bool vm_frame_ok(const double* origin, double voxel) {
  auto fin = [](double x) { return x > -INFINITY && x < INFINITY; };       // false for NaN
  return origin && voxel > 0.0 && fin(voxel) && fin(origin[0]) && fin(origin[1]) && fin(origin[2]);
}
static inline bool vm_integrate_shape_ok(int64_t points_capacity, int n_obs) {
  return points_capacity >= 0 && points_capacity < (1ll << 31) && n_obs >= 1 && n_obs <= VM_MAX_OBS;
}

}  // namespace egonn
