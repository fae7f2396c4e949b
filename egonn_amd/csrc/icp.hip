// ICP refinement of scan pairs on the device: voxel-grid downsample, exact radius-limited nearest neighbour over two full
// clouds, N-point rigid fit.  The reference runs Open3D through misc/point_clouds.py:31-62 (voxel_down_sample(0.1), then
// registration_icp, point-to-point, max distance 1.2, ICPConvergenceCriteria(max_iteration)); Open3D is not part of the
// reference tree, so the rules are restated from its documentation [recall] (DESIGN.md "ICP refinement"):
//
//   downsample   mb = min over the (cropped) points - voxel/2 per axis (fp64); idx = floor((p - mb) / voxel); one output point
//                per occupied voxel = fp64 mean of its points summed in input order; output order ascending (ix, iy, iz).
//   evaluation   under T: j(i) = nearest target point of T s_i by fp64 squared distance (ties: lowest index); i is a
//                correspondence iff d2 < max_dist^2 (strict); fitness = n_corr / n_source; rmse = sqrt(sum d2 / n_corr).
//   round k      U = least-squares rigid transform (no scale, det +1) of {T_k s_i} onto {t_j(i)}; T_k+1 = U T_k; evaluate;
//                stop if |d fitness| < eps_f and |d rmse| < eps_r.  The source is always transformed from the ORIGINAL points
//                by the cumulative T_k (Open3D transforms its working copy round after round).
//
// Kernels.  Once per call: icp_setup_kernel (target bounds -> grid origin and cell edge, T_0, EMPTY pairs), icp_key_kernel
// (cell key of every target point, Morton key of every source point under T_0), two segmented radix sorts (sort.hip),
// icp_gather_kernel (points in sorted order).  Per round icp_search_kernel + icp_finish_kernel:
//
//   search   a workgroup owns 256 consecutive source points of the Morton order (neighbours in space; a rigid motion keeps
//            them neighbours, so the order of T_0 serves every round).  It transforms them by T_k, takes their bounding box
//            padded by max_dist, converts it to a clamped range of target cells, finds per (x, y) column of that range the
//            run of target points by binary search in the sorted cell keys (a column's z range is one contiguous run), and
//            streams the runs through LDS in tiles of 256 points; every lane keeps (best d2, best j, its coordinates) in
//            registers.  Every target point within max_dist of one of the workgroup's points lies in the padded box, so the
//            result is the exact nearest neighbour within max_dist.  The workgroup leaves 17 fp64 partials: n_corr, sum d2,
//            the two coordinate sums and the 3 x 3 sum of products.
//   finish   one wave per pair: the partials in ascending workgroup order, fitness / rmse, the stop decision, Horn's
//            closed form (largest eigenvector of the 4 x 4 matrix by cyclic Jacobi; a unit quaternion is a proper
//            rotation, which is the reflection-corrected least-squares solution), T_k+1 = U T_k.
//
// The partition (256 points per workgroup, counted from the pair's own first point), the summation order and the Jacobi
// schedule are fixed, there are no floating-point atomics: a pair's result has the same bits alone, in any batch and at any
// batch position.  The launch sequence is fixed by max_iteration; a stopped pair sets a flag and its later workgroups
// return at once: no host synchronisation, capturable.
#include "../../include/egonn_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int ICP_WG = 256;
static constexpr int ICP_NPART = 17;              // n_corr, sum d2, sum p (3), sum q (3), sum p q^T (9)
static constexpr int DS_BITS = 21;                // voxel index bits per axis
static constexpr int ICP_CELL_MAX = 65535;        // cell index bits per axis: 16
static constexpr uint64_t DS_INVALID = ~0ull;     // key of a dropped / out-of-cloud point (valid keys have bit 63 clear)


// segment of position i: the largest c in [0, C) with clip(off[c]) <= i, or -1 when i is beyond the last segment
__device__ static inline int icp_segment(const int64_t* __restrict__ off, int C, int64_t n, int64_t i) {
  if (i >= clipi(off[C], n)) return -1;
  int lo = 0, hi = C - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (clipi(off[mid], n) <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// first position in [lo, hi) whose key is >= k
__device__ static inline int icp_lower_bound(const uint64_t* __restrict__ keys, int lo, int hi, uint64_t k) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------ voxel downsample
__device__ static inline bool ds_keep(const float* __restrict__ p, const double* crop) {
  // preprocess_pointcloud: x > min_x, x <= max_x, ...; a NaN bound compares false on both sides of !(..): no bound
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  return !(x <= crop[0]) && !(x > crop[1]) && !(y <= crop[2]) && !(y > crop[3]) && !(z <= crop[4]) && !(z > crop[5]);
}

struct DsCrop { double b[6]; };

__global__ __launch_bounds__(ICP_WG) void ds_min_kernel(const float* __restrict__ pts, int64_t n, const int64_t* __restrict__ off,
                                                        int C, DsCrop crop, double voxel, double* __restrict__ mins,
                                                        int32_t* __restrict__ status) {
  __shared__ double s_m[3][ICP_WG];
  const int c = blockIdx.x, t = threadIdx.x;
  const int64_t lo = clipi(off[c], n), hi = clipi(off[c + 1], n);
  double m[3] = {INFINITY, INFINITY, INFINITY};
  for (int64_t i = lo + t; i < hi; i += ICP_WG) {
    const float* p = pts + i * 3;
    if (ds_keep(p, crop.b)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) m[k] = fmin(m[k], (double)p[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) s_m[k][t] = m[k];
  __syncthreads();
  for (int s = ICP_WG / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s_m[k][t] = fmin(s_m[k][t], s_m[k][t + s]);
    }
    __syncthreads();
  }
  if (t < 3) mins[c * 3 + t] = s_m[t][0] - voxel / 2.0;
  if (t == 0) status[c] = 0;
}

__global__ __launch_bounds__(ICP_WG) void ds_key_kernel(const float* __restrict__ pts, int64_t n, const int64_t* __restrict__ off,
                                                        int C, DsCrop crop, double voxel, const double* __restrict__ mins,
                                                        uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                        int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * ICP_WG + threadIdx.x;
  if (i >= n) return;
  uint64_t key = DS_INVALID;
  const int c = icp_segment(off, C, n, i);
  if (c >= 0) {
    const float* p = pts + i * 3;
    if (ds_keep(p, crop.b)) {
      uint64_t idx[3];
      bool ok = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double f = floor(((double)p[k] - mins[c * 3 + k]) / voxel);
        ok = ok && f >= 0.0 && f < (double)(1 << DS_BITS);     // false for NaN / inf as well
        idx[k] = ok ? (uint64_t)f : 0ull;
      }
      if (ok) key = (idx[0] << (2 * DS_BITS)) | (idx[1] << DS_BITS) | idx[2];
      else atomicOr(&status[c], EGONN_ICP_STATUS_RANGE);
    }
  }
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

// is sorted position i the first point of a voxel?  (c = its cloud, -1 = none)
__device__ static inline bool ds_is_head(const uint64_t* __restrict__ keys, const int64_t* __restrict__ off, int C, int64_t n,
                                         const int32_t* __restrict__ status, int64_t i, int* cloud) {
  if (i >= n) return false;
  const int c = icp_segment(off, C, n, i);
  *cloud = c;
  if (c < 0 || (status[c] & EGONN_ICP_STATUS_RANGE)) return false;
  const uint64_t k = keys[i];
  if (k == DS_INVALID) return false;
  return i == clipi(off[c], n) || keys[i - 1] != k;
}

__global__ __launch_bounds__(ICP_WG) void ds_count_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ off, int C,
                                                          int64_t n, const int32_t* __restrict__ status,
                                                          int32_t* __restrict__ blockcnt) {
  __shared__ int s_w[4];
  const int t = threadIdx.x;
  int c;
  const bool head = ds_is_head(keys, off, C, n, status, (int64_t)blockIdx.x * ICP_WG + t, &c);
  const unsigned long long bal = __ballot(head);
  if ((t & 63) == 0) s_w[t >> 6] = __popcll(bal);
  __syncthreads();
  if (t == 0) blockcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// one workgroup: exclusive scan of the block counts (in place), then the output offsets of the clouds
__global__ __launch_bounds__(ICP_WG) void ds_scan_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ off, int C,
                                                         int64_t n, const int32_t* __restrict__ status, int32_t* __restrict__ blockcnt,
                                                         int nb, int64_t* __restrict__ out_off) {
  __shared__ int s_sum[ICP_WG];
  const int t = threadIdx.x;
  const int per = (nb + ICP_WG - 1) / ICP_WG;
  const int b0 = min(t * per, nb), b1 = min(b0 + per, nb);
  int s = 0;
  for (int b = b0; b < b1; ++b) s += blockcnt[b];
  s_sum[t] = s;
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int k = 0; k < ICP_WG; ++k) {
      const int v = s_sum[k];
      s_sum[k] = acc;
      acc += v;
    }
  }
  __syncthreads();
  int acc = s_sum[t];
  for (int b = b0; b < b1; ++b) {
    const int v = blockcnt[b];
    blockcnt[b] = acc;
    acc += v;
  }
  __threadfence_block();
  __syncthreads();
  for (int c = t; c <= C; c += ICP_WG) {
    const int64_t pos = clipi(off[c], n);
    const int64_t b = pos / ICP_WG;
    int64_t cnt = 0;
    if (b < nb) {
      cnt = blockcnt[b];
      int dummy;
      for (int64_t i = b * ICP_WG; i < pos; ++i) cnt += ds_is_head(keys, off, C, n, status, i, &dummy) ? 1 : 0;
    } else if (nb > 0) {          // pos == n == nb * 256: everything
      cnt = blockcnt[nb - 1];
      int dummy;
      for (int64_t i = (int64_t)(nb - 1) * ICP_WG; i < pos; ++i) cnt += ds_is_head(keys, off, C, n, status, i, &dummy) ? 1 : 0;
    }
    out_off[c] = cnt;
  }
}

__global__ __launch_bounds__(ICP_WG) void ds_write_kernel(const float* __restrict__ pts, const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ vals, const int64_t* __restrict__ off, int C,
                                                          int64_t n, const int32_t* __restrict__ status,
                                                          const int32_t* __restrict__ blockpre, double* __restrict__ out_pts,
                                                          int32_t* __restrict__ out_cnt) {
  __shared__ int s_w[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t i = (int64_t)blockIdx.x * ICP_WG + t;
  int c = -1;
  const bool head = ds_is_head(keys, off, C, n, status, i, &c);
  const unsigned long long bal = __ballot(head);
  if (lane == 0) s_w[w] = __popcll(bal);
  __syncthreads();
  if (!head) return;
  int64_t o = blockpre[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; ++k) o += s_w[k];
  if (o >= n) return;                         // cannot happen (heads <= points); keeps the store in bounds regardless
  const int64_t hi = clipi(off[c + 1], n);
  const uint64_t key = keys[i];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int cnt = 0;
  for (int64_t j = i; j < hi && keys[j] == key; ++j) {      // the sort is stable: ascending input order
    const uint32_t v = vals[j];
    if ((int64_t)v >= n) break;
    sx += (double)pts[(int64_t)v * 3];
    sy += (double)pts[(int64_t)v * 3 + 1];
    sz += (double)pts[(int64_t)v * 3 + 2];
    ++cnt;
  }
  const double k = (double)(cnt > 0 ? cnt : 1);
  out_pts[o * 3] = sx / k;
  out_pts[o * 3 + 1] = sy / k;
  out_pts[o * 3 + 2] = sz / k;
  if (out_cnt) out_cnt[o] = cnt;
}

struct DsLayout {
  size_t keys0, keys1, vals0, vals1, mins, blockcnt, sort, sort_bytes, total;
};
static DsLayout ds_layout(int64_t n, int C) {
  DsLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
  const size_t m = (size_t)(n > 0 ? n : 1);
  L.keys0 = take(m * 8), L.keys1 = take(m * 8), L.vals0 = take(m * 4), L.vals1 = take(m * 4);
  L.mins = take((size_t)C * 3 * 8);
  L.blockcnt = take((size_t)(cdiv((int64_t)m, ICP_WG) + 1) * 4);
  // + 512: the sort carves two arrays out of this span and Arena::alloc aligns each carve to 256
  L.sort_bytes = align_up(radix_sort_segments_scratch_bytes((int64_t)m, C) + 512, 256);
  L.sort = take(L.sort_bytes);
  L.total = o;
  return L;
}

// ------------------------------------------------------------------ ICP
struct IcpPair {
  double R[9], t[3];        // T_k
  double org[3], h;         // target grid: origin (min corner) and cell edge
  double prev_fit, prev_rmse;
  int64_t so, to;           // first source / target point
  int32_t ns, nt;
  int32_t dim[3];           // cells per axis
  int32_t done, status, pad;
};

__device__ static inline int icp_cell(double f, int dim) {     // floor value -> clamped cell index; NaN -> 0
  return !(f > 0.0) ? 0 : (f >= (double)(dim - 1) ? dim - 1 : (int)f);
}

__global__ __launch_bounds__(ICP_WG) void icp_setup_kernel(const double* __restrict__ tgt, int64_t nt_cap,
                                                           const int64_t* __restrict__ soff, const int64_t* __restrict__ toff,
                                                           int64_t ns_cap, int P, const double* __restrict__ T_init, double max_dist,
                                                           IcpPair* __restrict__ pairs, int32_t* __restrict__ wg0,
                                                           double* __restrict__ T_out, double* __restrict__ fitness,
                                                           double* __restrict__ rmse, int32_t* __restrict__ iterations,
                                                           int32_t* __restrict__ status, double* __restrict__ T_trace, int max_it) {
  __shared__ double s_lo[3][ICP_WG], s_hi[3][ICP_WG];
  const int p = blockIdx.x, t = threadIdx.x;
  const int64_t so = clipi(soff[p], ns_cap), se = clipi(soff[p + 1], ns_cap);
  const int64_t to = clipi(toff[p], nt_cap), te = clipi(toff[p + 1], nt_cap);
  const int64_t ns = se > so ? se - so : 0, nt = te > to ? te - to : 0;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = to + t; i < to + nt; i += ICP_WG) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = tgt[i * 3 + k];
      lo[k] = fmin(lo[k], v);
      hi[k] = fmax(hi[k], v);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) s_lo[k][t] = lo[k], s_hi[k][t] = hi[k];
  __syncthreads();
  for (int s = ICP_WG / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s_lo[k][t] = fmin(s_lo[k][t], s_lo[k][t + s]);
        s_hi[k][t] = fmax(s_hi[k][t], s_hi[k][t + s]);
      }
    }
    __syncthreads();
  }
  if (t != 0) return;
  IcpPair q;
  double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (T_init)
    for (int k = 0; k < 16; ++k) T[k] = T_init[(size_t)p * 16 + k];
  for (int r = 0; r < 3; ++r) {
    q.R[r * 3] = T[r * 4], q.R[r * 3 + 1] = T[r * 4 + 1], q.R[r * 3 + 2] = T[r * 4 + 2];
    q.t[r] = T[r * 4 + 3];
  }
  double ext = 0.0;
  for (int k = 0; k < 3; ++k) {
    q.org[k] = nt > 0 ? s_lo[k][0] : 0.0;
    const double e = nt > 0 ? s_hi[k][0] - s_lo[k][0] : 0.0;
    if (e > ext) ext = e;
  }
  double h = max_dist;                                  // any edge >= 0 is exact; max_dist keeps the padded box a few cells wide
  const double hmin = ext / (double)(ICP_CELL_MAX - 1);  // at most 2^16 cells per axis
  if (!(h >= hmin)) h = hmin;
  if (!(h > 0.0)) h = 1.0;
  q.h = h;
  for (int k = 0; k < 3; ++k) {
    const double f = nt > 0 ? floor((s_hi[k][0] - q.org[k]) / h) : 0.0;
    q.dim[k] = icp_cell(f, ICP_CELL_MAX + 1) + 1;
  }
  q.prev_fit = q.prev_rmse = 0.0;
  q.so = so, q.to = to, q.ns = (int32_t)ns, q.nt = (int32_t)nt;
  q.done = 0, q.status = 0, q.pad = 0;
  if (T_trace)
    for (int k = 0; k < 16; ++k) T_trace[((size_t)p * (max_it + 1)) * 16 + k] = k < 12 ? T[k] : (k == 15 ? 1.0 : 0.0);
  if (ns == 0 || nt == 0) {
    q.done = 1, q.status = EGONN_ICP_STATUS_EMPTY;
    for (int k = 0; k < 16; ++k) T_out[(size_t)p * 16 + k] = k < 12 ? T[k] : (k == 15 ? 1.0 : 0.0);
    fitness[p] = 0.0, rmse[p] = 0.0, iterations[p] = 0, status[p] = q.status;
  }
  pairs[p] = q;
  // first workgroup of the pair in the flat search grid: a function of the sizes of the pairs before it only
  int64_t w = 0;
  for (int b = 0; b < p; ++b) {
    const int64_t a = clipi(soff[b], ns_cap), e = clipi(soff[b + 1], ns_cap);
    w += e > a ? (e - a + ICP_WG - 1) / ICP_WG : 0;
  }
  wg0[p] = (int32_t)w;
  if (p == P - 1) wg0[P] = (int32_t)(w + (ns + ICP_WG - 1) / ICP_WG);
}

// side 0: cell key of every target point; side 1: Morton key of every source point's cell under T_0 (order only)
__global__ __launch_bounds__(ICP_WG) void icp_key_kernel(const double* __restrict__ pts, int64_t n, const int64_t* __restrict__ off,
                                                         int P, const IcpPair* __restrict__ pairs, int side,
                                                         uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * ICP_WG + threadIdx.x;
  if (i >= n) return;
  uint64_t key = 0;
  const int p = icp_segment(off, P, n, i);
  if (p >= 0) {
    const IcpPair* q = pairs + p;
    const double x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    if (side == 0) {
      const uint64_t cx = (uint64_t)icp_cell(floor((x - q->org[0]) / q->h), q->dim[0]);
      const uint64_t cy = (uint64_t)icp_cell(floor((y - q->org[1]) / q->h), q->dim[1]);
      const uint64_t cz = (uint64_t)icp_cell(floor((z - q->org[2]) / q->h), q->dim[2]);
      key = (cx << 32) | (cy << 16) | cz;
    } else {
      const double px = q->R[0] * x + q->R[1] * y + q->R[2] * z + q->t[0];
      const double py = q->R[3] * x + q->R[4] * y + q->R[5] * z + q->t[1];
      const double pz = q->R[6] * x + q->R[7] * y + q->R[8] * z + q->t[2];
      const uint32_t cx = (uint32_t)icp_cell(floor((px - q->org[0]) / q->h) + 16384.0, ICP_CELL_MAX + 1);
      const uint32_t cy = (uint32_t)icp_cell(floor((py - q->org[1]) / q->h) + 16384.0, ICP_CELL_MAX + 1);
      const uint32_t cz = (uint32_t)icp_cell(floor((pz - q->org[2]) / q->h) + 16384.0, ICP_CELL_MAX + 1);
      key = morton3(cx, cy, cz);
    }
  }
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(ICP_WG) void icp_gather_kernel(const double* __restrict__ pts, int64_t n, const int64_t* __restrict__ off,
                                                            int P, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            double* __restrict__ out_pts, int32_t* __restrict__ out_idx,
                                                            uint64_t* __restrict__ out_keys) {
  const int64_t i = (int64_t)blockIdx.x * ICP_WG + threadIdx.x;
  if (i >= n) return;
  const int p = icp_segment(off, P, n, i);
  if (p < 0) return;
  const int64_t first = clipi(off[p], n);
  int64_t v = (int64_t)vals[i];
  if (v < first || v >= clipi(off[p + 1], n)) v = first;      // cannot happen after a sort of the segment; keeps reads in bounds
  out_pts[i * 3] = pts[v * 3], out_pts[i * 3 + 1] = pts[v * 3 + 1], out_pts[i * 3 + 2] = pts[v * 3 + 2];
  out_idx[i] = (int32_t)(v - first);
  if (out_keys) out_keys[i] = keys[i];
}

__global__ __launch_bounds__(ICP_WG) void icp_search_kernel(const IcpPair* __restrict__ pairs, const int32_t* __restrict__ wg0, int P,
                                                            const double* __restrict__ sq, const int32_t* __restrict__ si,
                                                            const double* __restrict__ tq, const int32_t* __restrict__ tj,
                                                            const uint64_t* __restrict__ tkey, double max_dist,
                                                            double* __restrict__ partial, int32_t* __restrict__ corr) {
  __shared__ double s_q[3][ICP_WG];
  __shared__ int s_j[ICP_WG];
  __shared__ int s_start[ICP_WG], s_pre[ICP_WG + 1];
  __shared__ double s_red[ICP_NPART][4];
  __shared__ double s_box[6][4];
  __shared__ int s_wsum[4];
  const int flat = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  // pair of this workgroup: the largest p with wg0[p] <= flat
  int p = 0;
  {
    int lo = 0, hi = P - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (wg0[mid] <= flat) lo = mid; else hi = mid - 1;
    }
    p = lo;
  }
  const IcpPair* q = pairs + p;
  const int chunk = flat - wg0[p];
  const int ns = q->ns, nt = q->nt;
  if (q->done || chunk < 0 || (int64_t)chunk * ICP_WG >= ns) return;          // workgroup-uniform
  const int row = chunk * ICP_WG + t;
  const bool valid = row < ns;
  const int64_t so = q->so, to = q->to;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (valid) {
    const double x = sq[(so + row) * 3], y = sq[(so + row) * 3 + 1], z = sq[(so + row) * 3 + 2];
    px = q->R[0] * x + q->R[1] * y + q->R[2] * z + q->t[0];
    py = q->R[3] * x + q->R[4] * y + q->R[5] * z + q->t[1];
    pz = q->R[6] * x + q->R[7] * y + q->R[8] * z + q->t[2];
  }
  // bounding box of the workgroup's transformed points
  {
    double b[6] = {valid ? px : INFINITY, valid ? py : INFINITY, valid ? pz : INFINITY,
                   valid ? px : -INFINITY, valid ? py : -INFINITY, valid ? pz : -INFINITY};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        b[k] = fmin(b[k], __shfl_xor(b[k], o, 64));
        b[3 + k] = fmax(b[3 + k], __shfl_xor(b[3 + k], o, 64));
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) s_box[k][w] = b[k];
    }
  }
  __syncthreads();
  int clo[3], chi[3];
  {
    // the pad is max_dist and a little more: the roundings of the box, of the cell function and of d2 are ~1e-14 m
    const double pad = max_dist * (1.0 + 0x1p-20) + 0x1p-20;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double lo = fmin(fmin(s_box[k][0], s_box[k][1]), fmin(s_box[k][2], s_box[k][3]));
      const double hi = fmax(fmax(s_box[3 + k][0], s_box[3 + k][1]), fmax(s_box[3 + k][2], s_box[3 + k][3]));
      const double flo = floor((lo - pad - q->org[k]) / q->h), fhi = floor((hi + pad - q->org[k]) / q->h);
      // a box wholly outside the grid gets an empty range: its cells hold nothing
      clo[k] = flo > (double)(q->dim[k] - 1) ? q->dim[k] : icp_cell(flo, q->dim[k]);
      chi[k] = fhi < 0.0 ? -1 : icp_cell(fhi, q->dim[k]);
      if (!(lo <= hi)) clo[k] = 0, chi[k] = -1;         // no finite point
    }
  }
  const double md2 = max_dist * max_dist;
  double best = INFINITY, bqx = 0.0, bqy = 0.0, bqz = 0.0;
  int bj = -1;
  const int ny = chi[1] - clo[1] + 1, nx = chi[0] - clo[0] + 1;
  const int64_t ncol = (nx > 0 && ny > 0 && chi[2] >= clo[2]) ? (int64_t)nx * ny : 0;
  const uint64_t* keys = tkey + to;
  for (int64_t c0 = 0; c0 < ncol; c0 += ICP_WG) {
    // runs of target points of up to 256 (x, y) columns of the cell range: one contiguous run per column
    const int64_t c = c0 + t;
    int start = 0, len = 0;
    if (c < ncol) {
      const uint64_t x = (uint64_t)(clo[0] + (int)(c / ny)), y = (uint64_t)(clo[1] + (int)(c % ny));
      const uint64_t k0 = (x << 32) | (y << 16) | (uint64_t)clo[2], k1 = (x << 32) | (y << 16) | (uint64_t)chi[2];
      start = icp_lower_bound(keys, 0, nt, k0);
      len = icp_lower_bound(keys, start, nt, k1 + 1) - start;
    }
    int incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    __syncthreads();                                   // the previous batch's tiles have been consumed
    if (lane == 63) s_wsum[w] = incl;
    __syncthreads();
    int pre = incl - len;
    for (int k = 0; k < w; ++k) pre += s_wsum[k];
    s_start[t] = start;
    s_pre[t] = pre;
    if (t == ICP_WG - 1) s_pre[ICP_WG] = pre + len;
    __syncthreads();
    const int total = s_pre[ICP_WG];
    for (int e0 = 0; e0 < total; e0 += ICP_WG) {
      const int e = e0 + t;
      if (e < total) {
        int lo = 0, hi = ICP_WG - 1;                   // the largest column with s_pre[column] <= e
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (s_pre[mid] <= e) lo = mid; else hi = mid - 1;
        }
        int idx = s_start[lo] + (e - s_pre[lo]);
        idx = idx < 0 ? 0 : (idx >= nt ? nt - 1 : idx);
        s_q[0][t] = tq[(to + idx) * 3], s_q[1][t] = tq[(to + idx) * 3 + 1], s_q[2][t] = tq[(to + idx) * 3 + 2];
        s_j[t] = tj[to + idx];
      }
      __syncthreads();
      const int cnt = min(ICP_WG, total - e0);
      if (valid) {
        for (int k = 0; k < cnt; ++k) {                // every lane reads the same address: LDS broadcast
          const double qx = s_q[0][k], qy = s_q[1][k], qz = s_q[2][k];
          const double dx = px - qx, dy = py - qy, dz = pz - qz;
          const double d2 = dx * dx + dy * dy + dz * dz;
          const int j = s_j[k];
          if (d2 < best || (d2 == best && j < bj)) best = d2, bj = j, bqx = qx, bqy = qy, bqz = qz;
        }
      }
      __syncthreads();
    }
  }
  const bool is_corr = valid && bj >= 0 && best < md2;
  if (corr && valid) {
    const int32_t orig = si[so + row];
    if (orig >= 0 && orig < ns) corr[so + orig] = is_corr ? bj : -1;
  }
  double v[ICP_NPART];
  v[0] = is_corr ? 1.0 : 0.0;
  v[1] = is_corr ? best : 0.0;
  const double a[3] = {is_corr ? px : 0.0, is_corr ? py : 0.0, is_corr ? pz : 0.0};
  const double b[3] = {is_corr ? bqx : 0.0, is_corr ? bqy : 0.0, is_corr ? bqz : 0.0};
#pragma unroll
  for (int k = 0; k < 3; ++k) v[2 + k] = a[k], v[5 + k] = b[k];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[8 + r * 3 + c] = a[r] * b[c];
#pragma unroll
  for (int k = 0; k < ICP_NPART; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);      // a fixed tree
    if (lane == 0) s_red[k][w] = v[k];
  }
  __syncthreads();
  if (t < ICP_NPART) partial[(size_t)flat * ICP_NPART + t] = ((s_red[t][0] + s_red[t][1]) + s_red[t][2]) + s_red[t][3];
}

// largest eigenvector of the symmetric 4 x 4 matrix A (cyclic Jacobi, fixed schedule): the unit quaternion (w, x, y, z)
__device__ static void icp_top_eigenvector(double A[4][4], double* qv) {
  double V[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {
    double offd = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i + 1; j < 4; ++j) offd += fabs(A[i][j]);
    if (offd == 0.0) break;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i + 1; j < 4; ++j) {
        const double apq = A[i][j];
        if (apq == 0.0) continue;
        const double theta = (A[j][j] - A[i][i]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {              // A <- A J
          const double aki = A[k][i], akj = A[k][j];
          A[k][i] = c * aki - s * akj;
          A[k][j] = s * aki + c * akj;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {              // A <- J^T A
          const double aik = A[i][k], ajk = A[j][k];
          A[i][k] = c * aik - s * ajk;
          A[j][k] = s * aik + c * ajk;
        }
        A[i][j] = A[j][i] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double vki = V[k][i], vkj = V[k][j];
          V[k][i] = c * vki - s * vkj;
          V[k][j] = s * vki + c * vkj;
        }
      }
  }
  int m = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (A[i][i] > A[m][m]) m = i;
  double nrm = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double e = V[k][0];
    if (m == 1) e = V[k][1];
    if (m == 2) e = V[k][2];
    if (m == 3) e = V[k][3];
    qv[k] = e;
    nrm += e * e;
  }
  nrm = 1.0 / sqrt(nrm);
#pragma unroll
  for (int k = 0; k < 4; ++k) qv[k] *= nrm;
}

__global__ __launch_bounds__(64) void icp_finish_kernel(IcpPair* __restrict__ pairs, const int32_t* __restrict__ wg0,
                                                        const double* __restrict__ partial, int round, int max_it, double eps_fit,
                                                        double eps_rmse, double* __restrict__ T_out, double* __restrict__ fitness,
                                                        double* __restrict__ rmse, int32_t* __restrict__ iterations,
                                                        int32_t* __restrict__ status, double* __restrict__ T_trace,
                                                        double* __restrict__ eval_trace) {
  __shared__ double s[ICP_NPART];
  const int p = blockIdx.x, t = threadIdx.x;
  IcpPair* q = pairs + p;
  if (q->done) return;
  const int nwg = (q->ns + ICP_WG - 1) / ICP_WG, first = wg0[p];
  if (t < ICP_NPART) {
    double acc = 0.0;
    for (int c = 0; c < nwg; ++c) acc += partial[(size_t)(first + c) * ICP_NPART + t];     // ascending workgroups
    s[t] = acc;
  }
  __syncthreads();
  if (t != 0) return;
  const double n = s[0];
  const double fit = n / (double)q->ns, e_rmse = n > 0.0 ? sqrt(s[1] / n) : 0.0;
  int stop = 0, st = q->status;
  if (round >= 1 && fabs(fit - q->prev_fit) < eps_fit && fabs(e_rmse - q->prev_rmse) < eps_rmse) stop = 1;
  else if (round >= max_it) stop = 1, st |= EGONN_ICP_STATUS_MAX_ITER;
  else if (n < 3.0) stop = 1, st |= EGONN_ICP_STATUS_FEW_CORR;
  if (eval_trace) {
    double* e = eval_trace + ((size_t)p * (max_it + 1) + round) * 3;
    e[0] = n, e[1] = s[1], e[2] = (double)stop;
  }
  if (stop) {
    double* To = T_out + (size_t)p * 16;
    for (int r = 0; r < 3; ++r) To[r * 4] = q->R[r * 3], To[r * 4 + 1] = q->R[r * 3 + 1], To[r * 4 + 2] = q->R[r * 3 + 2], To[r * 4 + 3] = q->t[r];
    To[12] = To[13] = To[14] = 0.0, To[15] = 1.0;
    fitness[p] = fit, rmse[p] = e_rmse, iterations[p] = round, status[p] = st;
    q->status = st;
    q->done = 1;
    return;
  }
  // Horn: S = sum (p - pm)(q - qm)^T, the 4 x 4 matrix N, its largest eigenvector
  double pm[3], qm[3], S[3][3];
  for (int k = 0; k < 3; ++k) pm[k] = s[2 + k] / n, qm[k] = s[5 + k] / n;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) S[r][c] = s[8 + r * 3 + c] - n * pm[r] * qm[c];
  double N[4][4];
  N[0][0] = S[0][0] + S[1][1] + S[2][2];
  N[1][1] = S[0][0] - S[1][1] - S[2][2];
  N[2][2] = -S[0][0] + S[1][1] - S[2][2];
  N[3][3] = -S[0][0] - S[1][1] + S[2][2];
  N[0][1] = N[1][0] = S[1][2] - S[2][1];
  N[0][2] = N[2][0] = S[2][0] - S[0][2];
  N[0][3] = N[3][0] = S[0][1] - S[1][0];
  N[1][2] = N[2][1] = S[0][1] + S[1][0];
  N[1][3] = N[3][1] = S[2][0] + S[0][2];
  N[2][3] = N[3][2] = S[1][2] + S[2][1];
  double qv[4];
  icp_top_eigenvector(N, qv);
  const double qw = qv[0], qx = qv[1], qy = qv[2], qz = qv[3];
  double U[9];
  U[0] = 1.0 - 2.0 * (qy * qy + qz * qz), U[1] = 2.0 * (qx * qy - qw * qz), U[2] = 2.0 * (qx * qz + qw * qy);
  U[3] = 2.0 * (qx * qy + qw * qz), U[4] = 1.0 - 2.0 * (qx * qx + qz * qz), U[5] = 2.0 * (qy * qz - qw * qx);
  U[6] = 2.0 * (qx * qz - qw * qy), U[7] = 2.0 * (qy * qz + qw * qx), U[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
  double ut[3], Rn[9], tn[3];
  for (int r = 0; r < 3; ++r) ut[r] = qm[r] - (U[r * 3] * pm[0] + U[r * 3 + 1] * pm[1] + U[r * 3 + 2] * pm[2]);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = U[r * 3] * q->R[c] + U[r * 3 + 1] * q->R[3 + c] + U[r * 3 + 2] * q->R[6 + c];
    tn[r] = U[r * 3] * q->t[0] + U[r * 3 + 1] * q->t[1] + U[r * 3 + 2] * q->t[2] + ut[r];
  }
  for (int k = 0; k < 9; ++k) q->R[k] = Rn[k];
  for (int k = 0; k < 3; ++k) q->t[k] = tn[k];
  q->prev_fit = fit, q->prev_rmse = e_rmse;
  if (T_trace) {
    double* To = T_trace + ((size_t)p * (max_it + 1) + round + 1) * 16;
    for (int r = 0; r < 3; ++r) To[r * 4] = Rn[r * 3], To[r * 4 + 1] = Rn[r * 3 + 1], To[r * 4 + 2] = Rn[r * 3 + 2], To[r * 4 + 3] = tn[r];
    To[12] = To[13] = To[14] = 0.0, To[15] = 1.0;
  }
}

struct IcpLayout {
  size_t pairs, wg0, keys0, keys1, vals0, vals1, tq, tj, tkey, sq, si, partial, sort, sort_bytes, total;
  int64_t n_wg;
};
static IcpLayout icp_layout(int64_t ns, int64_t nt, int P) {
  IcpLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
  const size_t a = (size_t)(ns > 0 ? ns : 1), b = (size_t)(nt > 0 ? nt : 1), m = a > b ? a : b;
  L.n_wg = cdiv((int64_t)a, ICP_WG) + P;
  L.pairs = take((size_t)P * sizeof(IcpPair));
  L.wg0 = take((size_t)(P + 1) * 4);
  L.keys0 = take(m * 8), L.keys1 = take(m * 8), L.vals0 = take(m * 4), L.vals1 = take(m * 4);
  L.tq = take(b * 24), L.tj = take(b * 4), L.tkey = take(b * 8);
  L.sq = take(a * 24), L.si = take(a * 4);
  L.partial = take((size_t)L.n_wg * ICP_NPART * 8);
  // + 512: the sort carves two arrays out of this span and Arena::alloc aligns each carve to 256
  L.sort_bytes = align_up(radix_sort_segments_scratch_bytes((int64_t)m, P) + 512, 256);
  L.sort = take(L.sort_bytes);
  L.total = o;
  return L;
}

}  // namespace egonn

using namespace egonn;

API int64_t egonn_voxel_downsample_scratch_bytes(int64_t n, int n_clouds) {
  if (n < 0 || n >= (1ll << 31) || n_clouds < 1 || n_clouds > EGONN_MAX_BATCH) return -1;
  return (int64_t)ds_layout(n, n_clouds).total;
}

API int egonn_voxel_downsample(const float* points, int64_t n, const int64_t* offsets, int n_clouds, double voxel_size,
                               const float* crop, double* out_points, int64_t* out_offsets, int32_t* out_counts, int32_t* status,
                               void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(n >= 0 && n < (1ll << 31) && n_clouds >= 1 && n_clouds <= EGONN_MAX_BATCH, EGONN_ERR_INVALID,
                "voxel_downsample: bad shape (n=%lld, n_clouds=%d; n_clouds <= %d)", (long long)n, n_clouds, EGONN_MAX_BATCH);
  EGONN_REQUIRE(voxel_size > 0.0 && voxel_size < 1e18, EGONN_ERR_INVALID, "voxel_downsample: bad voxel_size");
  EGONN_REQUIRE(offsets && out_offsets && status && scratch && (n == 0 || (points && out_points)), EGONN_ERR_INVALID,
                "voxel_downsample: null pointer");
  const DsLayout L = ds_layout(n, n_clouds);
  EGONN_REQUIRE(scratch_bytes >= (int64_t)L.total && ((uintptr_t)scratch & 255) == 0, EGONN_ERR_INVALID,
                "voxel_downsample: scratch needs %lld bytes, 256-byte aligned", (long long)L.total);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)scratch;
  DsCrop cr;
  for (int k = 0; k < 6; ++k) cr.b[k] = crop ? (double)crop[k] : (double)NAN;
  double* mins = (double*)(base + L.mins);
  int32_t* blockcnt = (int32_t*)(base + L.blockcnt);
  hipLaunchKernelGGL(ds_min_kernel, dim3((unsigned)n_clouds), dim3(ICP_WG), 0, st, points, n, offsets, n_clouds, cr, voxel_size, mins,
                     status);
  const int nb = (int)cdiv(n, ICP_WG);
  uint64_t* keys = (uint64_t*)(base + L.keys0);
  uint32_t* vals = (uint32_t*)(base + L.vals0);
  if (n > 0) {
    hipLaunchKernelGGL(ds_key_kernel, dim3((unsigned)nb), dim3(ICP_WG), 0, st, points, n, offsets, n_clouds, cr, voxel_size, mins, keys,
                       vals, status);
    Arena sort_ws = Arena::view(base + L.sort, L.sort_bytes);
    EGONN_TRY(radix_sort_segments(sort_ws, keys, vals, (uint64_t*)(base + L.keys1), (uint32_t*)(base + L.vals1), n, offsets, n_clouds,
                                  64, st, &keys, &vals));
    hipLaunchKernelGGL(ds_count_kernel, dim3((unsigned)nb), dim3(ICP_WG), 0, st, keys, offsets, n_clouds, n, status, blockcnt);
  }
  hipLaunchKernelGGL(ds_scan_kernel, dim3(1), dim3(ICP_WG), 0, st, keys, offsets, n_clouds, n, status, blockcnt, nb, out_offsets);
  if (n > 0)
    hipLaunchKernelGGL(ds_write_kernel, dim3((unsigned)nb), dim3(ICP_WG), 0, st, points, keys, vals, offsets, n_clouds, n, status,
                       blockcnt, out_points, out_counts);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int64_t egonn_icp_scratch_bytes(int64_t n_src, int64_t n_tgt, int n_pairs) {
  if (n_src < 0 || n_tgt < 0 || n_src >= (1ll << 31) || n_tgt >= (1ll << 31) || n_pairs < 1 || n_pairs > EGONN_MAX_BATCH) return -1;
  return (int64_t)icp_layout(n_src, n_tgt, n_pairs).total;
}

API int egonn_icp_pairs(const double* src, int64_t n_src, const int64_t* src_offsets, const double* tgt, int64_t n_tgt,
                        const int64_t* tgt_offsets, int n_pairs, const double* T_init, double max_dist, int max_iteration,
                        double eps_fitness, double eps_rmse, double* T, double* fitness, double* inlier_rmse, int32_t* iterations,
                        int32_t* status, double* T_trace, double* eval_trace, int32_t* corr, void* scratch, int64_t scratch_bytes,
                        void* stream) {
  EGONN_REQUIRE(n_src >= 0 && n_tgt >= 0 && n_src < (1ll << 31) && n_tgt < (1ll << 31) && n_pairs >= 1 && n_pairs <= EGONN_MAX_BATCH,
                EGONN_ERR_INVALID, "icp_pairs: bad shape (n_src=%lld, n_tgt=%lld, n_pairs=%d; n_pairs <= %d)", (long long)n_src,
                (long long)n_tgt, n_pairs, EGONN_MAX_BATCH);
  EGONN_REQUIRE(max_dist > 0.0 && max_dist < 1e18, EGONN_ERR_INVALID, "icp_pairs: bad distance threshold");
  EGONN_REQUIRE(max_iteration >= 0 && max_iteration <= 100000, EGONN_ERR_INVALID, "icp_pairs: max_iteration %d outside [0, 100000]",
                max_iteration);
  EGONN_REQUIRE(eps_fitness >= 0.0 && eps_rmse >= 0.0, EGONN_ERR_INVALID, "icp_pairs: negative convergence threshold");
  EGONN_REQUIRE(src_offsets && tgt_offsets && T && fitness && inlier_rmse && iterations && status && scratch &&
                    (n_src == 0 || src) && (n_tgt == 0 || tgt),
                EGONN_ERR_INVALID, "icp_pairs: null pointer");
  const IcpLayout L = icp_layout(n_src, n_tgt, n_pairs);
  EGONN_REQUIRE(scratch_bytes >= (int64_t)L.total && ((uintptr_t)scratch & 255) == 0, EGONN_ERR_INVALID,
                "icp_pairs: scratch needs %lld bytes, 256-byte aligned", (long long)L.total);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)scratch;
  IcpPair* pairs = (IcpPair*)(base + L.pairs);
  int32_t* wg0 = (int32_t*)(base + L.wg0);
  const size_t rounds = (size_t)max_iteration + 1;
  if (T_trace) HIP_CHECK(hipMemsetAsync(T_trace, 0, (size_t)n_pairs * rounds * 16 * sizeof(double), st));
  if (eval_trace) HIP_CHECK(hipMemsetAsync(eval_trace, 0, (size_t)n_pairs * rounds * 3 * sizeof(double), st));
  if (corr && n_src > 0) HIP_CHECK(hipMemsetAsync(corr, 0xFF, (size_t)n_src * sizeof(int32_t), st));
  hipLaunchKernelGGL(icp_setup_kernel, dim3((unsigned)n_pairs), dim3(ICP_WG), 0, st, tgt, n_tgt, src_offsets, tgt_offsets, n_src,
                     n_pairs, T_init, max_dist, pairs, wg0, T, fitness, inlier_rmse, iterations, status, T_trace, max_iteration);
  HIP_CHECK(hipGetLastError());
  if (n_src == 0 || n_tgt == 0) return EGONN_OK;         // every pair is EMPTY
  double* tq = (double*)(base + L.tq);
  int32_t* tj = (int32_t*)(base + L.tj);
  uint64_t* tkey = (uint64_t*)(base + L.tkey);
  double* sq = (double*)(base + L.sq);
  int32_t* si = (int32_t*)(base + L.si);
  double* partial = (double*)(base + L.partial);
  Arena sort_ws = Arena::view(base + L.sort, L.sort_bytes);
  for (int side = 0; side < 2; ++side) {
    const double* pts = side == 0 ? tgt : src;
    const int64_t n = side == 0 ? n_tgt : n_src;
    const int64_t* off = side == 0 ? tgt_offsets : src_offsets;
    uint64_t* keys = (uint64_t*)(base + L.keys0);
    uint32_t* vals = (uint32_t*)(base + L.vals0);
    const unsigned nb = (unsigned)cdiv(n, ICP_WG);
    hipLaunchKernelGGL(icp_key_kernel, dim3(nb), dim3(ICP_WG), 0, st, pts, n, off, n_pairs, pairs, side, keys, vals);
    EGONN_TRY(radix_sort_segments(sort_ws, keys, vals, (uint64_t*)(base + L.keys1), (uint32_t*)(base + L.vals1), n, off, n_pairs, 48,
                                  st, &keys, &vals));
    hipLaunchKernelGGL(icp_gather_kernel, dim3(nb), dim3(ICP_WG), 0, st, pts, n, off, n_pairs, keys, vals, side == 0 ? tq : sq,
                       side == 0 ? tj : si, side == 0 ? tkey : (uint64_t*)nullptr);
  }
  for (int k = 0; k <= max_iteration; ++k) {
    hipLaunchKernelGGL(icp_search_kernel, dim3((unsigned)L.n_wg), dim3(ICP_WG), 0, st, pairs, wg0, n_pairs, sq, si, tq, tj, tkey,
                       max_dist, partial, corr);
    hipLaunchKernelGGL(icp_finish_kernel, dim3((unsigned)n_pairs), dim3(64), 0, st, pairs, wg0, partial, k, max_iteration, eps_fitness,
                       eps_rmse, T, fitness, inlier_rmse, iterations, status, T_trace, eval_trace);
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
