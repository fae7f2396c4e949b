// Training-tuple generation on the device: the link between "a sequence of scans with poses" and what the training step
// consumes (datasets/mulran/generate_training_tuples.py, datasets/dataset_utils.py:83-88,210-232 of the reference).
//
//   egonn_radius_count / egonn_radius_fill   the radius search over pose positions (sklearn KDTree.query_radius there)
//   egonn_pair_masks                         positives_mask / negatives_mask of a batch (the double loop over in_sorted_array)
//   egonn_relative_poses                     inv(m_b) @ m_a per pair, as the affine inverse with the difference taken first
//   egonn_gather_clouds                      picked clouds of a resident bank, back to back, as egonn_icp_pairs takes them
//
// Rules every kernel here keeps: geometry in fp64 with contraction off (the products and sums below round one by one, so the
// numpy restatement in tests/tuples_data.py gives the same bits), integer atomics only (status words), no host
// synchronisation, outputs sized by capacities with a device status word.
//
// Radius join.  j is a neighbour of i iff  dx = qx_i - mx_j, dy = qy_i - my_j, dx*dx + dy*dy <= r*r  (each operation rounded
// to fp64; r*r is formed on the host, which is the same rounding).  A NaN coordinate fails every comparison: it is never a
// neighbour and has none.  A wave owns RJ_ROWS query rows; the workgroup streams the reference positions through LDS in tiles of
// 256 and every wave walks a tile in pieces of 64, lane l testing j = piece + l.  The ballot of a test is the row's hits in
// ascending j, its popcount below the lane the hit's slot behind the row's running count: a row comes out ascending by
// construction and nothing is sorted.  The count pass is the same loop without the stores.
#include "../../include/egonn_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int RJ_WG = 256;                 // 4 waves
static constexpr int RJ_ROWS = 8;                 // query rows per wave
static constexpr int RJ_WG_ROWS = RJ_ROWS * (RJ_WG / 64);
static constexpr int RJ_MAX_RADII = 4;
static constexpr int64_t RJ_MAX_N = 1ll << 24;
static constexpr int TUPLES_MAX_PICK = 4096;
static constexpr int GATHER_WG = 256;
static constexpr int GATHER_PER_THREAD = TUPLES_MAX_PICK / GATHER_WG;
static constexpr int GATHER_SLICES = 8;           // workgroups that share one picked cloud

struct RjRadii { double r2[RJ_MAX_RADII]; };

template <bool FILL, int NR>
__global__ __launch_bounds__(RJ_WG) void radius_kernel(const double* __restrict__ q, int64_t nq, const double* __restrict__ m,
                                                        int64_t nm, RjRadii rr, int exclude_mask, int32_t* __restrict__ counts,
                                                        const int64_t* __restrict__ off, int32_t* __restrict__ idx, int64_t cap,
                                                        int32_t* __restrict__ status) {
  __shared__ double sx[RJ_WG], sy[RJ_WG];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * (RJ_WG / 64) + wave) * RJ_ROWS;
  const unsigned long long below = (1ull << lane) - 1ull;
  double qx[RJ_ROWS], qy[RJ_ROWS];
  int64_t base[RJ_ROWS], end[RJ_ROWS];
  int32_t cnt[RJ_ROWS][NR];
#pragma unroll
  for (int k = 0; k < RJ_ROWS; ++k) {
    const int64_t row = row0 + k;
    const bool live = row < nq;                     // a row past the end carries NaN: it matches nothing
    qx[k] = live ? q[2 * row] : (double)NAN;
    qy[k] = live ? q[2 * row + 1] : (double)NAN;
    base[k] = (FILL && live) ? off[row] : 0;
    end[k] = (FILL && live) ? off[row + 1] : 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) cnt[k][r] = 0;
  }
  int bad = 0;
  for (int64_t tile = 0; tile < nm; tile += RJ_WG) {
    const int64_t jt = tile + threadIdx.x;
    sx[threadIdx.x] = jt < nm ? m[2 * jt] : (double)NAN;
    sy[threadIdx.x] = jt < nm ? m[2 * jt + 1] : (double)NAN;
    __syncthreads();
#pragma unroll
    for (int piece = 0; piece < RJ_WG; piece += 64) {
      if (tile + piece >= nm) break;                // uniform
      const int64_t j = tile + piece + lane;
      const double mx = sx[piece + lane], my = sy[piece + lane];
#pragma unroll
      for (int k = 0; k < RJ_ROWS; ++k) {
        const double dx = qx[k] - mx, dy = qy[k] - my;
        const double d2 = dx * dx + dy * dy;
        const bool self = j == row0 + k;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const bool hit = d2 <= rr.r2[r] && !(((exclude_mask >> r) & 1) && self);
          const unsigned long long mask = __ballot(hit);
          if (FILL && hit) {
            const int64_t slot = base[k] + cnt[k][r] + __popcll(mask & below);
            if (slot < 0 || slot >= cap) bad |= EGONN_TUPLES_STATUS_CAPACITY;
            else if (slot >= end[k]) bad |= EGONN_TUPLES_STATUS_BAD_OFFSETS;
            else idx[slot] = (int32_t)j;
          }
          cnt[k][r] += __popcll(mask);
        }
      }
    }
    __syncthreads();
  }
  if (FILL) {
#pragma unroll
    for (int k = 0; k < RJ_ROWS; ++k)               // a row with fewer hits than its offsets say would leave slots unwritten
      if (row0 + k < nq && base[k] + cnt[k][0] != end[k]) bad |= EGONN_TUPLES_STATUS_BAD_OFFSETS;
    if (bad) atomicOr(status, bad);
  } else if (lane == 0) {
#pragma unroll
    for (int k = 0; k < RJ_ROWS; ++k)
      if (row0 + k < nq)
#pragma unroll
        for (int r = 0; r < NR; ++r) counts[(int64_t)r * nq + row0 + k] = cnt[k][r];
  }
}

__global__ __launch_bounds__(256) void pair_masks_kernel(const int32_t* __restrict__ labels, int B, const int64_t* __restrict__ pos_off,
                                                          const int32_t* __restrict__ pos_idx, int64_t n_pos,
                                                          const int64_t* __restrict__ non_off, const int32_t* __restrict__ non_idx,
                                                          int64_t n_non, int64_t n_tuples, uint8_t* __restrict__ pos_mask,
                                                          uint8_t* __restrict__ neg_mask, int32_t* __restrict__ status) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * B) return;
  const int i = (int)(t / B), j = (int)(t % B);
  const int32_t li = labels[i], lj = labels[j];
  const bool ok_i = li >= 0 && li < n_tuples, ok_j = lj >= 0 && lj < n_tuples;
  int bad = (i == j && !ok_i) ? EGONN_TUPLES_STATUS_BAD_INDEX : 0;
  uint8_t p = 0, n = 0;
  if (ok_i && ok_j) {
    bool in_pos = false, in_non = false;
    for (int side = 0; side < 2; ++side) {
      const int64_t* off = side ? non_off : pos_off;
      const int32_t* idx = side ? non_idx : pos_idx;
      const int64_t cap = side ? n_non : n_pos;
      int64_t lo = off[li], hi = off[li + 1];
      const int64_t row_end = hi;
      if (lo < 0 || hi < lo || hi > cap) { bad |= EGONN_TUPLES_STATUS_BAD_OFFSETS; continue; }
      while (lo < hi) {                               // np.searchsorted, then the equality test of in_sorted_array
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (idx[mid] < lj) lo = mid + 1;
        else hi = mid;
      }
      const bool found = lo < row_end && idx[lo] == lj;
      if (side) in_non = found; else in_pos = found;
    }
    if (!(bad & EGONN_TUPLES_STATUS_BAD_OFFSETS)) p = in_pos ? 1 : 0, n = in_non ? 0 : 1;
  }
  pos_mask[t] = p;
  neg_mask[t] = n;
  if (bad) atomicOr(status, bad);
}

__global__ __launch_bounds__(256) void relative_poses_kernel(const double* __restrict__ poses, int64_t n, const int32_t* __restrict__ idx_a,
                                                              const int32_t* __restrict__ idx_b, int64_t P, int negate,
                                                              double* __restrict__ out, int32_t* __restrict__ status) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int64_t ia = idx_a[p], ib = idx_b[p];
  double o[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  int st = 0;
  if (ia < 0 || ia >= n || ib < 0 || ib >= n) st = EGONN_POSE_STATUS_BAD_INDEX;
  else {
    double a[16], b[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = poses[ia * 16 + k], b[k] = poses[ib * 16 + k];
    const bool rows = a[12] == 0.0 && a[13] == 0.0 && a[14] == 0.0 && a[15] == 1.0 && b[12] == 0.0 && b[13] == 0.0 && b[14] == 0.0 &&
                      b[15] == 1.0;
    if (!rows) st = EGONN_POSE_STATUS_BAD_ROW;
    else {
      // adjugate of R_b (cofactors transposed), row-major c[r][c]
      double c[9];
      c[0] = b[5] * b[10] - b[6] * b[9];
      c[1] = b[2] * b[9] - b[1] * b[10];
      c[2] = b[1] * b[6] - b[2] * b[5];
      c[3] = b[6] * b[8] - b[4] * b[10];
      c[4] = b[0] * b[10] - b[2] * b[8];
      c[5] = b[2] * b[4] - b[0] * b[6];
      c[6] = b[4] * b[9] - b[5] * b[8];
      c[7] = b[1] * b[8] - b[0] * b[9];
      c[8] = b[0] * b[5] - b[1] * b[4];
      const double det = (b[0] * c[0] + b[1] * c[3]) + b[2] * c[6];
      if (!(fabs(det) > 0.0) || !(fabs(det) < INFINITY)) st = EGONN_POSE_STATUS_SINGULAR;   // zero, NaN or infinite
      else {
        double inv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) inv[k] = c[k] / det;
        const double d[3] = {a[3] - b[3], a[7] - b[7], a[11] - b[11]};        // the difference first: UTM-sized terms cancel here
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int cc = 0; cc < 3; ++cc)
            o[r * 4 + cc] = (inv[r * 3] * a[cc] + inv[r * 3 + 1] * a[4 + cc]) + inv[r * 3 + 2] * a[8 + cc];
          const double t = (inv[r * 3] * d[0] + inv[r * 3 + 1] * d[1]) + inv[r * 3 + 2] * d[2];
          o[r * 4 + 3] = negate ? -t : t;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) out[p * 16 + k] = o[k];
  status[p] = st;
}

// one workgroup: sizes of the picked clouds, their exclusive scan, the capacity / index checks; all-zero offsets on failure
__global__ __launch_bounds__(GATHER_WG) void gather_offsets_kernel(const int64_t* __restrict__ bank_off, int64_t n_bank, int64_t n_clouds,
                                                                    const int32_t* __restrict__ pick, int n_pick, int64_t capacity,
                                                                    int64_t* __restrict__ out_off, int32_t* __restrict__ status) {
  __shared__ int64_t part[GATHER_WG];
  const int t = threadIdx.x;
  int64_t size[GATHER_PER_THREAD];
  int64_t sum = 0;
  int bad = 0;
#pragma unroll
  for (int k = 0; k < GATHER_PER_THREAD; ++k) {
    const int p = t * GATHER_PER_THREAD + k;
    size[k] = 0;
    if (p < n_pick) {
      const int64_t c = pick[p];
      if (c < 0 || c >= n_clouds) bad = 1;
      else {
        const int64_t lo = bank_off[c], hi = bank_off[c + 1];
        if (lo < 0 || hi < lo || hi > n_bank) bad = 1;
        else size[k] = hi - lo;
      }
    }
    sum += size[k];
  }
  part[t] = sum;
  __syncthreads();
  for (int s = 1; s < GATHER_WG; s <<= 1) {                    // inclusive scan of the 256 partial sums
    const int64_t v = t >= s ? part[t - s] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  const int64_t total = part[GATHER_WG - 1];
  int st = __syncthreads_or(bad) ? EGONN_TUPLES_STATUS_BAD_INDEX : 0;
  if (!st && total > capacity) st = EGONN_TUPLES_STATUS_CAPACITY;
  int64_t run = part[t] - sum;
#pragma unroll
  for (int k = 0; k < GATHER_PER_THREAD; ++k) {
    const int p = t * GATHER_PER_THREAD + k;
    if (p < n_pick) out_off[p] = st ? 0 : run;
    run += size[k];
  }
  if (t == 0) out_off[n_pick] = st ? 0 : total, *status = st;
}

__global__ __launch_bounds__(GATHER_WG) void gather_copy_kernel(const double* __restrict__ bank, const int64_t* __restrict__ bank_off,
                                                                 const int32_t* __restrict__ pick, const int64_t* __restrict__ out_off,
                                                                 double* __restrict__ out) {
  const int p = blockIdx.x;
  const int64_t dst = out_off[p] * 3, len = (out_off[p + 1] - out_off[p]) * 3;      // zero after a failed check: pick is not read
  if (len <= 0) return;
  const int64_t src = bank_off[pick[p]] * 3;
  for (int64_t k = (int64_t)blockIdx.y * GATHER_WG + threadIdx.x; k < len; k += (int64_t)GATHER_SLICES * GATHER_WG) out[dst + k] = bank[src + k];
}

static bool radii_ok(const double* radii, int n_radius) {
  if (!radii || n_radius < 1 || n_radius > RJ_MAX_RADII) return false;
  for (int r = 0; r < n_radius; ++r)
    if (!(radii[r] >= 0.0) || !(radii[r] < INFINITY)) return false;
  return true;
}

}  // namespace egonn

using namespace egonn;

API int egonn_radius_count(const double* query, int64_t nq, const double* ref, int64_t nm, const double* radii, int n_radius,
                           int exclude_self_mask, int32_t* counts, void* stream) {
  EGONN_REQUIRE(nq >= 0 && nm >= 0 && nq <= RJ_MAX_N && nm <= RJ_MAX_N, EGONN_ERR_INVALID,
                "radius_count: bad shape (nq=%lld, nm=%lld; both <= 2^24)", (long long)nq, (long long)nm);
  EGONN_REQUIRE(radii_ok(radii, n_radius), EGONN_ERR_INVALID, "radius_count: 1 to %d finite radii >= 0 required", RJ_MAX_RADII);
  EGONN_REQUIRE(exclude_self_mask >= 0 && exclude_self_mask < (1 << n_radius), EGONN_ERR_INVALID,
                "radius_count: exclude_self_mask names a radius that is not there");
  EGONN_REQUIRE(exclude_self_mask == 0 || (query == ref && nq == nm), EGONN_ERR_INVALID,
                "radius_count: exclude_self needs query and reference to be the same array");
  EGONN_REQUIRE((nq == 0 || (query && counts)) && (nm == 0 || ref), EGONN_ERR_INVALID, "radius_count: null pointer");
  if (nq == 0) return EGONN_OK;
  RjRadii rr;
  for (int r = 0; r < RJ_MAX_RADII; ++r) rr.r2[r] = r < n_radius ? radii[r] * radii[r] : -1.0;
  const dim3 grid((unsigned)cdiv(nq, RJ_WG_ROWS)), wg(RJ_WG);
  hipStream_t st = (hipStream_t)stream;
#define RJ_COUNT(NR)                                                                                                              \
  hipLaunchKernelGGL((radius_kernel<false, NR>), grid, wg, 0, st, query, nq, ref, nm, rr, exclude_self_mask, counts,               \
                     (const int64_t*)nullptr, (int32_t*)nullptr, (int64_t)0, (int32_t*)nullptr)
  switch (n_radius) {
    case 1: RJ_COUNT(1); break;
    case 2: RJ_COUNT(2); break;
    case 3: RJ_COUNT(3); break;
    default: RJ_COUNT(4); break;
  }
#undef RJ_COUNT
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_radius_fill(const double* query, int64_t nq, const double* ref, int64_t nm, double radius, int exclude_self,
                          const int64_t* offsets, int32_t* indices, int64_t capacity, int32_t* status, void* stream) {
  EGONN_REQUIRE(nq >= 0 && nm >= 0 && nq <= RJ_MAX_N && nm <= RJ_MAX_N, EGONN_ERR_INVALID,
                "radius_fill: bad shape (nq=%lld, nm=%lld; both <= 2^24)", (long long)nq, (long long)nm);
  EGONN_REQUIRE(radii_ok(&radius, 1), EGONN_ERR_INVALID, "radius_fill: a finite radius >= 0 required");
  EGONN_REQUIRE(!exclude_self || (query == ref && nq == nm), EGONN_ERR_INVALID,
                "radius_fill: exclude_self needs query and reference to be the same array");
  EGONN_REQUIRE(capacity >= 0 && status && (capacity == 0 || indices) && (nq == 0 || (query && offsets)) && (nm == 0 || ref),
                EGONN_ERR_INVALID, "radius_fill: null pointer or negative capacity");
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (nq == 0) return EGONN_OK;
  RjRadii rr;
  for (int r = 0; r < RJ_MAX_RADII; ++r) rr.r2[r] = r == 0 ? radius * radius : -1.0;
  hipLaunchKernelGGL((radius_kernel<true, 1>), dim3((unsigned)cdiv(nq, RJ_WG_ROWS)), dim3(RJ_WG), 0, st, query, nq, ref, nm, rr,
                     exclude_self ? 1 : 0, (int32_t*)nullptr, offsets, indices, capacity, status);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_pair_masks(const int32_t* labels, int batch_size, const int64_t* pos_offsets, const int32_t* pos_indices, int64_t n_pos,
                         const int64_t* non_offsets, const int32_t* non_indices, int64_t n_non, int64_t n_tuples,
                         uint8_t* positives_mask, uint8_t* negatives_mask, int32_t* status, void* stream) {
  EGONN_REQUIRE(batch_size >= 1 && batch_size <= EGONN_MAX_BATCH, EGONN_ERR_INVALID, "pair_masks: batch size %d outside [1, %d]",
                batch_size, EGONN_MAX_BATCH);
  EGONN_REQUIRE(n_tuples >= 0 && n_tuples < (1ll << 31) && n_pos >= 0 && n_non >= 0, EGONN_ERR_INVALID, "pair_masks: bad table sizes");
  EGONN_REQUIRE(labels && pos_offsets && non_offsets && positives_mask && negatives_mask && status && (n_pos == 0 || pos_indices) &&
                    (n_non == 0 || non_indices),
                EGONN_ERR_INVALID, "pair_masks: null pointer");
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  const int64_t n = (int64_t)batch_size * batch_size;
  hipLaunchKernelGGL(pair_masks_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, labels, batch_size, pos_offsets, pos_indices, n_pos,
                     non_offsets, non_indices, n_non, n_tuples, positives_mask, negatives_mask, status);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_relative_poses(const double* poses, int64_t n_poses, const int32_t* idx_a, const int32_t* idx_b, int64_t n_pairs,
                             int negate_translation, double* out, int32_t* status, void* stream) {
  EGONN_REQUIRE(n_poses >= 0 && n_poses < (1ll << 31) && n_pairs >= 0 && n_pairs < (1ll << 31), EGONN_ERR_INVALID,
                "relative_poses: bad shape (n_poses=%lld, n_pairs=%lld)", (long long)n_poses, (long long)n_pairs);
  EGONN_REQUIRE((n_poses == 0 || poses) && (n_pairs == 0 || (idx_a && idx_b && out && status)), EGONN_ERR_INVALID,
                "relative_poses: null pointer");
  if (n_pairs == 0) return EGONN_OK;
  hipLaunchKernelGGL(relative_poses_kernel, dim3((unsigned)cdiv(n_pairs, 256)), dim3(256), 0, (hipStream_t)stream, poses, n_poses, idx_a,
                     idx_b, n_pairs, negate_translation ? 1 : 0, out, status);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_gather_clouds(const double* bank, int64_t n_bank, const int64_t* bank_offsets, int64_t n_clouds, const int32_t* pick,
                            int n_pick, double* out, int64_t capacity, int64_t* out_offsets, int32_t* status, void* stream) {
  EGONN_REQUIRE(n_bank >= 0 && n_clouds >= 0 && n_clouds < (1ll << 31) && n_pick >= 1 && n_pick <= TUPLES_MAX_PICK && capacity >= 0,
                EGONN_ERR_INVALID, "gather_clouds: bad shape (n_bank=%lld, n_clouds=%lld, n_pick=%d <= %d, capacity=%lld)",
                (long long)n_bank, (long long)n_clouds, n_pick, TUPLES_MAX_PICK, (long long)capacity);
  EGONN_REQUIRE(bank_offsets && pick && out_offsets && status && (n_bank == 0 || bank) && (capacity == 0 || out), EGONN_ERR_INVALID,
                "gather_clouds: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gather_offsets_kernel, dim3(1), dim3(GATHER_WG), 0, st, bank_offsets, n_bank, n_clouds, pick, n_pick, capacity,
                     out_offsets, status);
  if (capacity > 0 && n_bank > 0)
    hipLaunchKernelGGL(gather_copy_kernel, dim3((unsigned)n_pick, GATHER_SLICES), dim3(GATHER_WG), 0, st, bank, bank_offsets, pick,
                       out_offsets, out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
