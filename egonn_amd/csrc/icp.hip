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
// The loop around it (per-pair state, the flat grid of workgroups, the reduction tree, the ascending gather, stop and advance)
// is pair_loop.h, shared with ndt.hip; this file supplies the search, the two estimators' terms and steps, and the stop rule.
// The partition (256 points per workgroup, counted from the pair's own first point), the summation order and the Jacobi
// schedule are fixed, there are no floating-point atomics: a pair's result has the same bits alone, in any batch and at any
// batch position.  The launch sequence is fixed by max_iteration; a stopped pair sets a flag and its later workgroups
// return at once: no host synchronisation, capturable.
//
// Point-to-plane (icp(..., point2plane=True) of the reference) is the same loop with another estimator, a template parameter of
// the search and finish kernels: surface normals of the target by an exact k-nearest-neighbour search on the same grid
// (nrm_knn_kernel, further down), 29 partials per workgroup (A = sum J J^T, b = sum J r) and a 6 x 6 LDL^T solve per round
// (icp_plane_step).  The point-to-point instantiation is the code above, operation for operation.
#include "../../include/egonn_hip.h"
#include "common.h"
#include "compact.h"
#include "horn.h"
#include "jacobi3.h"
#include "pair_loop.h"
#include "plane_step.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int ICP_WG = PAIR_WG;
static constexpr int ICP_NPART = 17;              // n_corr, sum d2, sum p (3), sum q (3), sum p q^T (9)
static constexpr int ICP_NPART_PLANE = 29;        // n_corr, sum d2, sum J J^T (21 upper entries), sum J r (6)
static constexpr int NRM_KNN_MIN = 3, NRM_KNN_MAX = 32;
static constexpr double NRM_CELL = 0.5;           // start radius and cell edge of the normals' grid: 5 voxels of the 0.1 m downsample
static constexpr int DS_BITS = 21;               // voxel index bits per axis
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
  int c;
  const int heads = wg_count<ICP_WG>(ds_is_head(keys, off, C, n, status, (int64_t)blockIdx.x * ICP_WG + threadIdx.x, &c));
  if (threadIdx.x == 0) blockcnt[blockIdx.x] = heads;
}

// one workgroup: exclusive scan of the block counts (in place), then the output offsets of the clouds
__global__ __launch_bounds__(ICP_WG) void ds_scan_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ off, int C,
                                                         int64_t n, const int32_t* __restrict__ status, int32_t* __restrict__ blockcnt,
                                                         int nb, int64_t* __restrict__ out_off) {
  wg_scan<ICP_WG>(blockcnt, nb);
  __threadfence_block();
  __syncthreads();
  for (int c = threadIdx.x; c <= C; c += ICP_WG) {
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
  const int64_t i = (int64_t)blockIdx.x * ICP_WG + threadIdx.x;
  int c = -1;
  const bool head = ds_is_head(keys, off, C, n, status, i, &c);
  const int64_t o = (int64_t)blockpre[blockIdx.x] + wg_rank<ICP_WG>(__ballot(head));
  if (!head) return;
  if (o >= n) return;                        // cannot happen (heads <= points); keeps the store in bounds regardless
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

// the downsample's carves of the caller's scratch.  With scratch = nullptr only `total` means anything
struct DsSpan {
  uint64_t* keys[2];        // ping-pong buffers of the sort
  uint32_t* vals[2];
  double* mins;
  int32_t* blockcnt;
  Arena sort_ws;
  size_t total;
};
static DsSpan ds_span(void* scratch, int64_t n, int C) {
  DsSpan S;
  Carve c(scratch);
  const size_t m = (size_t)(n > 0 ? n : 1);
  for (int k = 0; k < 2; ++k) S.keys[k] = c.take<uint64_t>(m);
  for (int k = 0; k < 2; ++k) S.vals[k] = c.take<uint32_t>(m);
  S.mins = c.take<double>((size_t)C * 3);
  S.blockcnt = c.take<int32_t>((size_t)cdiv((int64_t)m, ICP_WG) + 1);
  S.sort_ws = c.sort_arena(radix_sort_segments_scratch_bytes((int64_t)m, C));
  S.total = c.total();
  return S;
}

// ------------------------------------------------------------------ ICP
struct IcpPair {            // the members pair_loop.h asks for, and the target grid; the order is the kernels' (see there)
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
  const int64_t to = clipi(toff[p], nt_cap), te = clipi(toff[p + 1], nt_cap);
  const int64_t nt = te > to ? te - to : 0;
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
  pair_begin(&q, soff, ns_cap, P, p, T_init, T_trace, max_it, wg0);
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
  q.to = to, q.nt = (int32_t)nt, q.pad = 0;
  if (T_out && (q.ns == 0 || nt == 0)) {                 // the normals have no pair outputs; an empty cloud has no workgroup
    pair_stop(&q, p, 0, EGONN_ICP_STATUS_EMPTY, T_out, iterations, status);
    fitness[p] = 0.0, rmse[p] = 0.0;
  }
  pairs[p] = q;
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
      double c[3];
      pair_apply(q, pts + i * 3, c);
      const uint32_t cx = (uint32_t)icp_cell(floor((c[0] - q->org[0]) / q->h) + 16384.0, ICP_CELL_MAX + 1);
      const uint32_t cy = (uint32_t)icp_cell(floor((c[1] - q->org[1]) / q->h) + 16384.0, ICP_CELL_MAX + 1);
      const uint32_t cz = (uint32_t)icp_cell(floor((c[2] - q->org[2]) / q->h) + 16384.0, ICP_CELL_MAX + 1);
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

struct IcpRange { int lo[3], hi[3]; };      // a clamped range of target cells, inclusive; hi < lo on an axis = empty

// bounding box of the workgroup's points (lanes with !valid have none): per-wave minima / maxima into s_box; a barrier follows
__device__ static inline void icp_wave_box(double (*s_box)[4], bool valid, double px, double py, double pz) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
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

// the cells of pair q that the box of s_box, padded by `reach`, touches.  The pad is the reach and a little more: the roundings
// of the box, of the cell function and of d2 are ~1e-14 m
__device__ static inline IcpRange icp_cell_range(const IcpPair* __restrict__ q, const double (*s_box)[4], double reach) {
  IcpRange rg;
  const double pad = reach * (1.0 + 0x1p-20) + 0x1p-20;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double lo = fmin(fmin(s_box[k][0], s_box[k][1]), fmin(s_box[k][2], s_box[k][3]));
    const double hi = fmax(fmax(s_box[3 + k][0], s_box[3 + k][1]), fmax(s_box[3 + k][2], s_box[3 + k][3]));
    const double flo = floor((lo - pad - q->org[k]) / q->h), fhi = floor((hi + pad - q->org[k]) / q->h);
    // a box wholly outside the grid gets an empty range: its cells hold nothing
    rg.lo[k] = flo > (double)(q->dim[k] - 1) ? q->dim[k] : icp_cell(flo, q->dim[k]);
    rg.hi[k] = fhi < 0.0 ? -1 : icp_cell(fhi, q->dim[k]);
    if (!(lo <= hi)) rg.lo[k] = 0, rg.hi[k] = -1;         // no finite point
  }
  return rg;
}

// Streams the target points of the cell range rg through LDS in tiles of 256 points and hands every one of them, in the
// order of the sorted cell keys, to visit(qx, qy, qz, j) of every lane with `take`.  Per (x, y) column of the range the run
// of target points is found by binary search in the sorted cell keys (a column's z range is one contiguous run).  Every
// barrier is workgroup-uniform: rg must be.  keys / nt: the sorted cell keys of the pair's target; to: its first point in
// tq / tj.
template <class Visit>
__device__ __forceinline__ void icp_stream_cells(const uint64_t* __restrict__ keys, int nt, const double* __restrict__ tq,
                                                 const int32_t* __restrict__ tj, int64_t to, const IcpRange& rg, bool take,
                                                 Visit&& visit) {
  __shared__ double s_q[3][ICP_WG];
  __shared__ int s_j[ICP_WG];
  __shared__ int s_start[ICP_WG], s_pre[ICP_WG + 1];
  __shared__ int s_wsum[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int ny = rg.hi[1] - rg.lo[1] + 1, nx = rg.hi[0] - rg.lo[0] + 1;
  const int64_t ncol = (nx > 0 && ny > 0 && rg.hi[2] >= rg.lo[2]) ? (int64_t)nx * ny : 0;
  for (int64_t c0 = 0; c0 < ncol; c0 += ICP_WG) {
    // runs of target points of up to 256 (x, y) columns of the cell range: one contiguous run per column
    const int64_t c = c0 + t;
    int start = 0, len = 0;
    if (c < ncol) {
      const uint64_t x = (uint64_t)(rg.lo[0] + (int)(c / ny)), y = (uint64_t)(rg.lo[1] + (int)(c % ny));
      const uint64_t k0 = (x << 32) | (y << 16) | (uint64_t)rg.lo[2], k1 = (x << 32) | (y << 16) | (uint64_t)rg.hi[2];
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
      if (take) {
        for (int k = 0; k < cnt; ++k) visit(s_q[0][k], s_q[1][k], s_q[2][k], s_j[k]);      // one address for all lanes: LDS broadcast
      }
      __syncthreads();
    }
  }
}

// EST 0: point-to-point, 17 partials (n_corr, sum d2, sum p, sum q, sum p q^T).  EST 1: point-to-plane, 29 partials (n_corr,
// sum d2, the 21 upper entries of sum J J^T row by row, the 6 of sum J r) with r = (p - q) . n, J = [p x n, n], n = the normal
// of the final nearest target, fetched once after the tile loop.
template <int EST>
__global__ __launch_bounds__(ICP_WG) void icp_search_kernel(const IcpPair* __restrict__ pairs, const int32_t* __restrict__ wg0, int P,
                                                            const double* __restrict__ sq, const int32_t* __restrict__ si,
                                                            const double* __restrict__ tq, const int32_t* __restrict__ tj,
                                                            const uint64_t* __restrict__ tkey, const double* __restrict__ tnrm,
                                                            double max_dist, double* __restrict__ partial,
                                                            int32_t* __restrict__ corr) {
  constexpr int NP = EST ? ICP_NPART_PLANE : ICP_NPART;
  __shared__ double s_red[NP][4];
  __shared__ double s_box[6][4];
  const int flat = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int p = pair_of(wg0, P, flat);
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
  icp_wave_box(s_box, valid, px, py, pz);              // of the workgroup's transformed points
  __syncthreads();
  const IcpRange rg = icp_cell_range(q, s_box, max_dist);
  const double md2 = max_dist * max_dist;
  double best = INFINITY, bqx = 0.0, bqy = 0.0, bqz = 0.0;
  int bj = -1;
  icp_stream_cells(tkey + to, nt, tq, tj, to, rg, valid, [&](double qx, double qy, double qz, int j) {
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < best || (d2 == best && j < bj)) best = d2, bj = j, bqx = qx, bqy = qy, bqz = qz;
  });
  const bool is_corr = valid && bj >= 0 && best < md2;
  if (corr && valid) {
    const int32_t orig = si[so + row];
    if (orig >= 0 && orig < ns) corr[so + orig] = is_corr ? bj : -1;
  }
  double v[NP];
  v[0] = is_corr ? 1.0 : 0.0;
  v[1] = is_corr ? best : 0.0;
  if constexpr (EST == 0) {
    const double a[3] = {is_corr ? px : 0.0, is_corr ? py : 0.0, is_corr ? pz : 0.0};
    const double b[3] = {is_corr ? bqx : 0.0, is_corr ? bqy : 0.0, is_corr ? bqz : 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) v[2 + k] = a[k], v[5 + k] = b[k];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[8 + r * 3 + c] = a[r] * b[c];
  } else {
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (is_corr) {                                       // bj is an index inside the pair's target (icp_gather_kernel)
      const int64_t j = to + (bj < nt ? bj : nt - 1);
      nx = tnrm[j * 3], ny = tnrm[j * 3 + 1], nz = tnrm[j * 3 + 2];
    }
    const double dx = px - bqx, dy = py - bqy, dz = pz - bqz;
    const double r = is_corr ? (dx * nx + dy * ny) + dz * nz : 0.0;
    double J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
    if (!is_corr) {
#pragma unroll
      for (int k = 0; k < 6; ++k) J[k] = 0.0;
    }
    int e = 2;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) v[e++] = J[a] * J[b];
#pragma unroll
    for (int a = 0; a < 6; ++a) v[23 + a] = J[a] * r;
  }
  pair_reduce<NP>(v, s_red, partial, flat, lane, w);
}

// icp_plane_step (plane_step.h): the 6 x 6 solve by LDL^T and the update it stands for, shared with ndt.hip

// EST as in icp_search_kernel.  One loop, two estimators: the evaluation, the stop rule and the traces are the same code.
template <int EST>
__global__ __launch_bounds__(64) void icp_finish_kernel(IcpPair* __restrict__ pairs, const int32_t* __restrict__ wg0,
                                                        const double* __restrict__ partial, int round, int max_it, double eps_fit,
                                                        double eps_rmse, double* __restrict__ T_out, double* __restrict__ fitness,
                                                        double* __restrict__ rmse, int32_t* __restrict__ iterations,
                                                        int32_t* __restrict__ status, double* __restrict__ T_trace,
                                                        double* __restrict__ eval_trace) {
  constexpr int NP = EST ? ICP_NPART_PLANE : ICP_NPART;
  __shared__ double s[NP];
  const int p = blockIdx.x, t = threadIdx.x;
  IcpPair* q = pairs + p;
  if (q->done) return;
  pair_gather<NP>(q, wg0[p], partial, s);
  if (t != 0) return;
  const double n = s[0];
  const double fit = n / (double)q->ns, e_rmse = n > 0.0 ? sqrt(s[1] / n) : 0.0;
  int stop = 0, st = q->status;
  double U[9], ut[3];
  if (round >= 1 && fabs(fit - q->prev_fit) < eps_fit && fabs(e_rmse - q->prev_rmse) < eps_rmse) stop = 1;
  else if (round >= max_it) stop = 1, st |= EGONN_ICP_STATUS_MAX_ITER;
  else if (n < (EST ? 6.0 : 3.0)) stop = 1, st |= EGONN_ICP_STATUS_FEW_CORR;
  else if constexpr (EST == 1) {
    if (!icp_plane_step(s, U, ut)) stop = 1, st |= EGONN_ICP_STATUS_SINGULAR;
  }
  if (eval_trace) {
    double* e = eval_trace + ((size_t)p * (max_it + 1) + round) * 3;
    e[0] = n, e[1] = s[1], e[2] = (double)stop;
  }
  if (stop) {
    fitness[p] = fit, rmse[p] = e_rmse;
    pair_stop(q, p, round, st, T_out, iterations, status);
    return;
  }
  if constexpr (EST == 0) {
    // Horn: S = sum (p - pm)(q - qm)^T, the 4 x 4 matrix N, its largest eigenvector
    double pm[3], qm[3], S[3][3];
    for (int k = 0; k < 3; ++k) pm[k] = s[2 + k] / n, qm[k] = s[5 + k] / n;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) S[r][c] = s[8 + r * 3 + c] - n * pm[r] * qm[c];
    horn_rotation(S, U);
    for (int r = 0; r < 3; ++r) ut[r] = qm[r] - (U[r * 3] * pm[0] + U[r * 3 + 1] * pm[1] + U[r * 3 + 2] * pm[2]);
  }
  q->prev_fit = fit, q->prev_rmse = e_rmse;
  pair_advance(q, p, round, max_it, U, ut, T_trace);
}

// ------------------------------------------------------------------ surface normals: exact k nearest neighbours, PCA
// Open3D's estimate_normals(KDTreeSearchParamKNN(knn)) [recall], restated (DESIGN.md "Point-to-plane ICP"):
//   neighbours   all points of the same cloud, the query itself included, by (d2, index) ascending with
//                d2 = (dx*dx + dy*dy) + dz*dz; the first m = min(knn, cloud size).
//   covariance   mean = (sum q) / m, C = sum (q - mean)(q - mean)^T / m, both summed in neighbour order.
//   normal       unit eigenvector of C's smallest eigenvalue (cyclic Jacobi, fixed schedule), flipped so that n . p <= 0
//                (toward the sensor at the origin); with n . p == 0 its first non-zero component is positive.
//                m < 3, a largest eigenvalue that is not > 0 or a non-finite value: (0, 0, 1).
// The grid is the ICP's with target = the cloud itself (icp_setup_kernel with T = identity, icp_key_kernel, the sorts,
// icp_gather_kernel).  A workgroup owns 256 Morton-consecutive points, pads their box by r and streams that cell range
// (icp_stream_cells); a lane is finished when it holds m entries and its m-th d2 is <= r^2: every closer point lay in the
// padded box, so the list is exact and a larger pass cannot change it.  While a lane is unfinished and the range does not
// cover the grid, r doubles and the unfinished lanes start over.  (d2, index) is a total order: the radius schedule, and
// with it the partition into workgroups, cannot change a result.

// one workgroup per cloud: RANGE if a coordinate is not finite, FEW_POINTS if the cloud has fewer than knn points
__global__ __launch_bounds__(ICP_WG) void nrm_status_kernel(const double* __restrict__ pts, int64_t n, const int64_t* __restrict__ off,
                                                            int knn, int32_t* __restrict__ status) {
  const int c = blockIdx.x, t = threadIdx.x;
  const int64_t lo = clipi(off[c], n), hi = clipi(off[c + 1], n);
  int bad = 0;
  for (int64_t i = lo + t; i < hi; i += ICP_WG)
    if (!(fabs(pts[i * 3]) < INFINITY && fabs(pts[i * 3 + 1]) < INFINITY && fabs(pts[i * 3 + 2]) < INFINITY)) bad = 1;
  bad = __syncthreads_or(bad);
  if (t == 0)
    status[c] = (bad ? EGONN_NORMALS_STATUS_RANGE : 0) | ((hi > lo ? hi - lo : 0) < knn ? EGONN_NORMALS_STATUS_FEW_POINTS : 0);
}

// nrm_jacobi3 (jacobi3.h): cyclic Jacobi on a symmetric 3 x 3 matrix, shared with ndt.hip

// K: the capacity of a lane's sorted list, kept in registers (every index below is a compile-time constant after unrolling)
template <int K>
__global__ __launch_bounds__(ICP_WG) void nrm_knn_kernel(const IcpPair* __restrict__ pairs, const int32_t* __restrict__ wg0, int P,
                                                         const double* __restrict__ pts, const double* __restrict__ sq,
                                                         const int32_t* __restrict__ si, const double* __restrict__ tq,
                                                         const int32_t* __restrict__ tj, const uint64_t* __restrict__ tkey, int knn,
                                                         const int32_t* __restrict__ status, double* __restrict__ normals,
                                                         int32_t* __restrict__ neighbors, double* __restrict__ eigenvalues) {
  __shared__ double s_box[6][4];
  const int flat = blockIdx.x, t = threadIdx.x;
  const int p = pair_of(wg0, P, flat);
  const IcpPair* q = pairs + p;
  const int chunk = flat - wg0[p];
  const int ns = q->ns;                                   // source = target = the cloud
  if (chunk < 0 || (int64_t)chunk * ICP_WG >= ns) return;  // workgroup-uniform; an empty cloud has no workgroup
  const int row = chunk * ICP_WG + t;
  const bool valid = row < ns;
  const int64_t so = q->so;
  int orig = valid ? si[so + row] : 0;
  orig = orig < 0 ? 0 : (orig >= ns ? ns - 1 : orig);
  double* nout = normals + (so + orig) * 3;
  if (status[p] & EGONN_NORMALS_STATUS_RANGE) {           // workgroup-uniform
    if (valid) {
      nout[0] = 0.0, nout[1] = 0.0, nout[2] = 1.0;
      if (neighbors)
        for (int s = 0; s < knn; ++s) neighbors[(so + orig) * knn + s] = -1;
      if (eigenvalues)
        for (int k = 0; k < 3; ++k) eigenvalues[(so + orig) * 3 + k] = 0.0;
    }
    return;
  }
  const int m = knn < ns ? knn : ns;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (valid) px = sq[(so + row) * 3], py = sq[(so + row) * 3 + 1], pz = sq[(so + row) * 3 + 2];
  icp_wave_box(s_box, valid, px, py, pz);
  __syncthreads();
  double ld[K];
  int lj[K];
  bool fin = !valid;
  // start radius: the cell edge, or an eighth of the box's longest side where the workgroup's points are sparse (256 points
  // of a surface at spacing s span ~16 s and their 20th neighbour lies ~2.5 s away).  Any start gives the same lists.
  double r = q->h;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double lo = fmin(fmin(s_box[k][0], s_box[k][1]), fmin(s_box[k][2], s_box[k][3]));
    const double hi = fmax(fmax(s_box[3 + k][0], s_box[3 + k][1]), fmax(s_box[3 + k][2], s_box[3 + k][3]));
    const double e = (hi - lo) * 0.125;
    if (e > r) r = e;                                      // false for NaN
  }
  for (int pass = 0; pass < 64; ++pass) {                  // r doubles: the grid has at most 2^16 cells per axis
    const IcpRange rg = icp_cell_range(q, s_box, r);
    const bool covers = rg.lo[0] == 0 && rg.lo[1] == 0 && rg.lo[2] == 0 && rg.hi[0] == q->dim[0] - 1 &&
                        rg.hi[1] == q->dim[1] - 1 && rg.hi[2] == q->dim[2] - 1;
    if (!fin) {
#pragma unroll
      for (int s = 0; s < K; ++s) ld[s] = INFINITY, lj[s] = 0x7fffffff;     // an empty slot: behind every point
    }
    icp_stream_cells(tkey + so, ns, tq, tj, so, rg, !fin, [&](double qx, double qy, double qz, int j) {
      const double dx = px - qx, dy = py - qy, dz = pz - qz;
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 < ld[K - 1] || (d2 == ld[K - 1] && j < lj[K - 1])) {
        bool here = true;                                  // the candidate sorts before slot s
#pragma unroll
        for (int s = K - 1; s >= 1; --s) {                 // compare and shift: slot s from slot s - 1, not yet touched
          const bool prev = d2 < ld[s - 1] || (d2 == ld[s - 1] && j < lj[s - 1]);
          ld[s] = prev ? ld[s - 1] : (here ? d2 : ld[s]);
          lj[s] = prev ? lj[s - 1] : (here ? j : lj[s]);
          here = prev;
        }
        if (here) ld[0] = d2, lj[0] = j;
      }
    });
    if (!fin) {
      double dm = INFINITY;
#pragma unroll
      for (int s = 0; s < K; ++s)
        if (s == m - 1) dm = ld[s];
      fin = dm <= r * r;
    }
    const int open = __syncthreads_or(fin ? 0 : 1);
    if (!open || covers) break;
    r = r + r;
  }
  if (!valid) return;
  // mean and covariance in neighbour order
  int cnt = 0;
  double mx = 0.0, my = 0.0, mz = 0.0;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    if (s < m && lj[s] < ns) {
      const double* g = pts + (so + lj[s]) * 3;
      mx += g[0], my += g[1], mz += g[2];
      ++cnt;
    }
  }
  const double dm = (double)(cnt > 0 ? cnt : 1);
  mx = mx / dm, my = my / dm, mz = mz / dm;
  double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    if (s < m && lj[s] < ns) {
      const double* g = pts + (so + lj[s]) * 3;
      const double ax = g[0] - mx, ay = g[1] - my, az = g[2] - mz;
      c00 += ax * ax, c01 += ax * ay, c02 += ax * az, c11 += ay * ay, c12 += ay * az, c22 += az * az;
    }
  }
  double A[3][3], V[3][3];
  A[0][0] = c00 / dm, A[1][1] = c11 / dm, A[2][2] = c22 / dm;
  A[0][1] = A[1][0] = c01 / dm, A[0][2] = A[2][0] = c02 / dm, A[1][2] = A[2][1] = c12 / dm;
  nrm_jacobi3(A, V);
  int lo = 0, hi = 0;
#pragma unroll
  for (int i = 1; i < 3; ++i) {
    if (A[i][i] < (lo == 0 ? A[0][0] : (lo == 1 ? A[1][1] : A[2][2]))) lo = i;
    if (A[i][i] > (hi == 0 ? A[0][0] : (hi == 1 ? A[1][1] : A[2][2]))) hi = i;
  }
  const double e0 = lo == 0 ? A[0][0] : (lo == 1 ? A[1][1] : A[2][2]), e2 = hi == 0 ? A[0][0] : (hi == 1 ? A[1][1] : A[2][2]);
  const int mid = lo == hi ? lo : 3 - lo - hi;
  const double e1 = mid == 0 ? A[0][0] : (mid == 1 ? A[1][1] : A[2][2]);
  double nx = lo == 0 ? V[0][0] : (lo == 1 ? V[0][1] : V[0][2]);
  double ny = lo == 0 ? V[1][0] : (lo == 1 ? V[1][1] : V[1][2]);
  double nz = lo == 0 ? V[2][0] : (lo == 1 ? V[2][1] : V[2][2]);
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  nx = nx / len, ny = ny / len, nz = nz / len;
  const double dot = (nx * px + ny * py) + nz * pz;
  const double lead = nx != 0.0 ? nx : (ny != 0.0 ? ny : nz);
  if (dot > 0.0 || (dot == 0.0 && lead < 0.0)) nx = -nx, ny = -ny, nz = -nz;
  const bool good = cnt >= 3 && e2 > 0.0 && fabs(e2) < INFINITY && fabs(nx) < 2.0 && fabs(ny) < 2.0 && fabs(nz) < 2.0;     // false for NaN
  nout[0] = good ? nx : 0.0, nout[1] = good ? ny : 0.0, nout[2] = good ? nz : 1.0;
  if (neighbors) {
#pragma unroll
    for (int s = 0; s < K; ++s)
      if (s < knn) neighbors[(so + orig) * knn + s] = (s < m && lj[s] < ns) ? lj[s] : -1;
  }
  if (eigenvalues) {
    double* ev = eigenvalues + (so + orig) * 3;
    ev[0] = e0, ev[1] = e1, ev[2] = e2;
  }
}

// The search grid that the ICP and the normals both build, as carves of the caller's scratch: the pairs and their workgroup
// table, the targets in cell order, the sources in Morton order under T_0, and what the two sorts need.  n_part: partial sums
// per workgroup (0: the normals have no rounds).  With scratch = nullptr only `total` means anything.
struct IcpGrid {
  int64_t n_wg;             // workgroups of the flat grid
  IcpPair* pairs;
  int32_t* wg0;
  double* partial;
  double *tq, *sq;          // points of the targets / sources in their order
  int32_t *tj, *si;         // their index inside the pair's own cloud
  uint64_t* tkey;           // cell keys of the targets
  uint64_t* keys[2];        // ping-pong buffers of the sorts
  uint32_t* vals[2];
  Arena sort_ws;
  size_t total;
};
static IcpGrid icp_grid(void* scratch, int64_t ns, int64_t nt, int P, int n_part) {
  IcpGrid G;
  Carve c(scratch);
  const size_t a = (size_t)(ns > 0 ? ns : 1), b = (size_t)(nt > 0 ? nt : 1), m = a > b ? a : b;
  const PairLayout L = pair_layout(c, (int64_t)a, P, sizeof(IcpPair));
  G.n_wg = L.n_wg, G.pairs = (IcpPair*)L.pairs, G.wg0 = L.wg0;
  for (int k = 0; k < 2; ++k) G.keys[k] = c.take<uint64_t>(m);
  for (int k = 0; k < 2; ++k) G.vals[k] = c.take<uint32_t>(m);
  G.tq = c.take<double>(b * 3), G.tj = c.take<int32_t>(b), G.tkey = c.take<uint64_t>(b);
  G.sq = c.take<double>(a * 3), G.si = c.take<int32_t>(a);
  G.partial = c.take<double>((size_t)L.n_wg * n_part);
  G.sort_ws = c.sort_arena(radix_sort_segments_scratch_bytes((int64_t)m, P));
  G.total = c.total();
  return G;
}

static bool icp_shape_ok(int64_t n_src, int64_t n_tgt, int n_pairs) {
  return n_src >= 0 && n_tgt >= 0 && n_src < (1ll << 31) && n_tgt < (1ll << 31) && n_pairs >= 1 && n_pairs <= EGONN_MAX_BATCH;
}

}  // namespace egonn

using namespace egonn;

API int64_t egonn_voxel_downsample_scratch_bytes(int64_t n, int n_clouds) {
  if (n < 0 || n >= (1ll << 31) || n_clouds < 1 || n_clouds > EGONN_MAX_BATCH) return -1;
  return (int64_t)ds_span(nullptr, n, n_clouds).total;
}

API int egonn_voxel_downsample(const float* points, int64_t n, const int64_t* offsets, int n_clouds, double voxel_size,
                               const float* crop, double* out_points, int64_t* out_offsets, int32_t* out_counts, int32_t* status,
                               void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(n >= 0 && n < (1ll << 31) && n_clouds >= 1 && n_clouds <= EGONN_MAX_BATCH, EGONN_ERR_INVALID,
                "voxel_downsample: bad shape (n=%lld, n_clouds=%d; n_clouds <= %d)", (long long)n, n_clouds, EGONN_MAX_BATCH);
  EGONN_REQUIRE(voxel_size > 0.0 && voxel_size < 1e18, EGONN_ERR_INVALID, "voxel_downsample: bad voxel_size");
  EGONN_REQUIRE(offsets && out_offsets && status && scratch && (n == 0 || (points && out_points)), EGONN_ERR_INVALID,
                "voxel_downsample: null pointer");
  DsSpan S = ds_span(scratch, n, n_clouds);
  EGONN_TRY(span_check("voxel_downsample", scratch, scratch_bytes, S.total));
  hipStream_t st = (hipStream_t)stream;
  DsCrop cr;
  for (int k = 0; k < 6; ++k) cr.b[k] = crop ? (double)crop[k] : (double)NAN;
  hipLaunchKernelGGL(ds_min_kernel, dim3((unsigned)n_clouds), dim3(ICP_WG), 0, st, points, n, offsets, n_clouds, cr, voxel_size, S.mins,
                     status);
  const int nb = (int)cdiv(n, ICP_WG);
  uint64_t* keys = S.keys[0];
  uint32_t* vals = S.vals[0];
  if (n > 0) {
    hipLaunchKernelGGL(ds_key_kernel, dim3((unsigned)nb), dim3(ICP_WG), 0, st, points, n, offsets, n_clouds, cr, voxel_size, S.mins, keys,
                       vals, status);
    EGONN_TRY(radix_sort_segments(S.sort_ws, keys, vals, S.keys[1], S.vals[1], n, offsets, n_clouds, 64, st, &keys, &vals));
    hipLaunchKernelGGL(ds_count_kernel, dim3((unsigned)nb), dim3(ICP_WG), 0, st, keys, offsets, n_clouds, n, status, S.blockcnt);
  }
  hipLaunchKernelGGL(ds_scan_kernel, dim3(1), dim3(ICP_WG), 0, st, keys, offsets, n_clouds, n, status, S.blockcnt, nb, out_offsets);
  if (n > 0)
    hipLaunchKernelGGL(ds_write_kernel, dim3((unsigned)nb), dim3(ICP_WG), 0, st, points, keys, vals, offsets, n_clouds, n, status,
                       S.blockcnt, out_points, out_counts);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// cell order of the targets (side 0: tq, tj, tkey) or Morton order of the sources under T_0 (side 1: sq, si) of every pair
static int icp_order_side(int side, const double* pts, int64_t n, const int64_t* off, int P, const IcpGrid& G, double* out_pts,
                          int32_t* out_idx, uint64_t* out_keys, hipStream_t st) {
  uint64_t* keys = G.keys[0];
  uint32_t* vals = G.vals[0];
  Arena ws = G.sort_ws;                                   // a view: every sort carves from its start
  const unsigned nb = (unsigned)cdiv(n, ICP_WG);
  hipLaunchKernelGGL(icp_key_kernel, dim3(nb), dim3(ICP_WG), 0, st, pts, n, off, P, G.pairs, side, keys, vals);
  EGONN_TRY(radix_sort_segments(ws, keys, vals, G.keys[1], G.vals[1], n, off, P, 48, st, &keys, &vals));
  hipLaunchKernelGGL(icp_gather_kernel, dim3(nb), dim3(ICP_WG), 0, st, pts, n, off, P, keys, vals, out_pts, out_idx, out_keys);
  return EGONN_OK;
}

// both sides of the grid, after icp_setup_kernel has filled G.pairs
static int icp_build_grid(const IcpGrid& G, const double* tgt, int64_t n_tgt, const int64_t* tgt_offsets, const double* src,
                          int64_t n_src, const int64_t* src_offsets, int P, hipStream_t st) {
  EGONN_TRY(icp_order_side(0, tgt, n_tgt, tgt_offsets, P, G, G.tq, G.tj, G.tkey, st));
  return icp_order_side(1, src, n_src, src_offsets, P, G, G.sq, G.si, nullptr, st);
}

// the ICP loop of both entry points; estimator (0: point-to-point, 1: point-to-plane) picks the instantiation of the two
// per-round kernels and is the one thing that tells the two calls apart
static int icp_run(int estimator, const char* who, const double* src, int64_t n_src, const int64_t* src_offsets,
                   const double* tgt, int64_t n_tgt, const int64_t* tgt_offsets, const double* tgt_normals, int n_pairs,
                   const double* T_init, double max_dist, int max_iteration, double eps_fitness, double eps_rmse, double* T,
                   double* fitness, double* inlier_rmse, int32_t* iterations, int32_t* status, double* T_trace, double* eval_trace,
                   int32_t* corr, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(icp_shape_ok(n_src, n_tgt, n_pairs), EGONN_ERR_INVALID,
                "%s: bad shape (n_src=%lld, n_tgt=%lld, n_pairs=%d; n_pairs <= %d)", who, (long long)n_src,
                (long long)n_tgt, n_pairs, EGONN_MAX_BATCH);
  EGONN_REQUIRE(max_dist > 0.0 && max_dist < 1e18, EGONN_ERR_INVALID, "%s: bad distance threshold", who);
  EGONN_REQUIRE(max_iteration >= 0 && max_iteration <= 100000, EGONN_ERR_INVALID, "%s: max_iteration %d outside [0, 100000]", who,
                max_iteration);
  EGONN_REQUIRE(eps_fitness >= 0.0 && eps_rmse >= 0.0, EGONN_ERR_INVALID, "%s: negative convergence threshold", who);
  EGONN_REQUIRE(src_offsets && tgt_offsets && T && fitness && inlier_rmse && iterations && status && scratch &&
                    (n_src == 0 || src) && (n_tgt == 0 || tgt),
                EGONN_ERR_INVALID, "%s: null pointer", who);
  EGONN_REQUIRE(!estimator || n_tgt == 0 || tgt_normals, EGONN_ERR_INVALID, "%s: null tgt_normals", who);
  const IcpGrid G = icp_grid(scratch, n_src, n_tgt, n_pairs, estimator ? ICP_NPART_PLANE : ICP_NPART);
  EGONN_TRY(span_check(who, scratch, scratch_bytes, G.total));
  hipStream_t st = (hipStream_t)stream;
  EGONN_TRY(pair_clear_traces(T_trace, eval_trace, 3, n_pairs, max_iteration, st));
  if (corr && n_src > 0) HIP_CHECK(hipMemsetAsync(corr, 0xFF, (size_t)n_src * sizeof(int32_t), st));
  hipLaunchKernelGGL(icp_setup_kernel, dim3((unsigned)n_pairs), dim3(ICP_WG), 0, st, tgt, n_tgt, src_offsets, tgt_offsets, n_src,
                     n_pairs, T_init, max_dist, G.pairs, G.wg0, T, fitness, inlier_rmse, iterations, status, T_trace, max_iteration);
  HIP_CHECK(hipGetLastError());
  if (n_src == 0 || n_tgt == 0) return EGONN_OK;         // every pair is EMPTY
  EGONN_TRY(icp_build_grid(G, tgt, n_tgt, tgt_offsets, src, n_src, src_offsets, n_pairs, st));
  const dim3 grid((unsigned)G.n_wg), one((unsigned)n_pairs);
  for (int k = 0; k <= max_iteration; ++k) {
    if (estimator) {
      hipLaunchKernelGGL(icp_search_kernel<1>, grid, dim3(ICP_WG), 0, st, G.pairs, G.wg0, n_pairs, G.sq, G.si, G.tq, G.tj, G.tkey,
                         tgt_normals, max_dist, G.partial, corr);
      hipLaunchKernelGGL(icp_finish_kernel<1>, one, dim3(64), 0, st, G.pairs, G.wg0, G.partial, k, max_iteration, eps_fitness, eps_rmse,
                         T, fitness, inlier_rmse, iterations, status, T_trace, eval_trace);
    } else {
      hipLaunchKernelGGL(icp_search_kernel<0>, grid, dim3(ICP_WG), 0, st, G.pairs, G.wg0, n_pairs, G.sq, G.si, G.tq, G.tj, G.tkey,
                         (const double*)nullptr, max_dist, G.partial, corr);
      hipLaunchKernelGGL(icp_finish_kernel<0>, one, dim3(64), 0, st, G.pairs, G.wg0, G.partial, k, max_iteration, eps_fitness, eps_rmse,
                         T, fitness, inlier_rmse, iterations, status, T_trace, eval_trace);
    }
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int64_t egonn_icp_scratch_bytes(int64_t n_src, int64_t n_tgt, int n_pairs) {
  if (!icp_shape_ok(n_src, n_tgt, n_pairs)) return -1;
  return (int64_t)icp_grid(nullptr, n_src, n_tgt, n_pairs, ICP_NPART).total;
}

API int egonn_icp_pairs(const double* src, int64_t n_src, const int64_t* src_offsets, const double* tgt, int64_t n_tgt,
                        const int64_t* tgt_offsets, int n_pairs, const double* T_init, double max_dist, int max_iteration,
                        double eps_fitness, double eps_rmse, double* T, double* fitness, double* inlier_rmse, int32_t* iterations,
                        int32_t* status, double* T_trace, double* eval_trace, int32_t* corr, void* scratch, int64_t scratch_bytes,
                        void* stream) {
  return icp_run(0, "icp_pairs", src, n_src, src_offsets, tgt, n_tgt, tgt_offsets, nullptr, n_pairs, T_init, max_dist, max_iteration,
                 eps_fitness, eps_rmse, T, fitness, inlier_rmse, iterations, status, T_trace, eval_trace, corr, scratch, scratch_bytes,
                 stream);
}

API int64_t egonn_icp_plane_scratch_bytes(int64_t n_src, int64_t n_tgt, int n_pairs) {
  if (!icp_shape_ok(n_src, n_tgt, n_pairs)) return -1;
  return (int64_t)icp_grid(nullptr, n_src, n_tgt, n_pairs, ICP_NPART_PLANE).total;
}

API int egonn_icp_plane_pairs(const double* src, int64_t n_src, const int64_t* src_offsets, const double* tgt, int64_t n_tgt,
                              const int64_t* tgt_offsets, const double* tgt_normals, int n_pairs, const double* T_init,
                              double max_dist, int max_iteration, double eps_fitness, double eps_rmse, double* T, double* fitness,
                              double* inlier_rmse, int32_t* iterations, int32_t* status, double* T_trace, double* eval_trace,
                              int32_t* corr, void* scratch, int64_t scratch_bytes, void* stream) {
  return icp_run(1, "icp_plane_pairs", src, n_src, src_offsets, tgt, n_tgt, tgt_offsets, tgt_normals, n_pairs, T_init, max_dist,
                 max_iteration, eps_fitness, eps_rmse, T, fitness, inlier_rmse, iterations, status, T_trace, eval_trace, corr, scratch,
                 scratch_bytes, stream);
}

API int64_t egonn_estimate_normals_scratch_bytes(int64_t n, int n_clouds) {
  if (!icp_shape_ok(n, n, n_clouds)) return -1;
  return (int64_t)icp_grid(nullptr, n, n, n_clouds, 0).total;
}

API int egonn_estimate_normals(const double* points, int64_t n, const int64_t* offsets, int n_clouds, int knn, double* normals,
                               int32_t* status, int32_t* neighbors, double* eigenvalues, void* scratch, int64_t scratch_bytes,
                               void* stream) {
  EGONN_REQUIRE(icp_shape_ok(n, n, n_clouds), EGONN_ERR_INVALID, "estimate_normals: bad shape (n=%lld, n_clouds=%d; n_clouds <= %d)",
                (long long)n, n_clouds, EGONN_MAX_BATCH);
  EGONN_REQUIRE(knn >= NRM_KNN_MIN && knn <= NRM_KNN_MAX, EGONN_ERR_INVALID, "estimate_normals: knn %d outside [%d, %d]", knn,
                NRM_KNN_MIN, NRM_KNN_MAX);
  EGONN_REQUIRE(offsets && status && scratch && (n == 0 || (points && normals)), EGONN_ERR_INVALID, "estimate_normals: null pointer");
  const IcpGrid G = icp_grid(scratch, n, n, n_clouds, 0);
  EGONN_TRY(span_check("estimate_normals", scratch, scratch_bytes, G.total));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nrm_status_kernel, dim3((unsigned)n_clouds), dim3(ICP_WG), 0, st, points, n, offsets, knn, status);
  HIP_CHECK(hipGetLastError());
  if (n == 0) return EGONN_OK;
  // the ICP's grid with source = target = the cloud, T = identity, the cell edge as the search radius and no pair outputs
  hipLaunchKernelGGL(icp_setup_kernel, dim3((unsigned)n_clouds), dim3(ICP_WG), 0, st, points, n, offsets, offsets, n, n_clouds,
                     (const double*)nullptr, NRM_CELL, G.pairs, G.wg0, (double*)nullptr, (double*)nullptr, (double*)nullptr,
                     (int32_t*)nullptr, (int32_t*)nullptr, (double*)nullptr, 0);
  EGONN_TRY(icp_build_grid(G, points, n, offsets, points, n, offsets, n_clouds, st));
  const dim3 grid((unsigned)G.n_wg);
  if (knn <= 20)
    hipLaunchKernelGGL(nrm_knn_kernel<20>, grid, dim3(ICP_WG), 0, st, G.pairs, G.wg0, n_clouds, points, G.sq, G.si, G.tq, G.tj, G.tkey, knn,
                       status, normals, neighbors, eigenvalues);
  else
    hipLaunchKernelGGL(nrm_knn_kernel<32>, grid, dim3(ICP_WG), 0, st, G.pairs, G.wg0, n_clouds, points, G.sq, G.si, G.tq, G.tj, G.tkey, knn,
                       status, normals, neighbors, eigenvalues);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
