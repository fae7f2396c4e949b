// A resident global voxel map: fuse posed scans (integrate), merge two sets of voxel records exactly (merge), crop submaps
// (select).  DESIGN.md §3.19; the arithmetic is stated once in include/egonn_hip.h ("voxel map") and restated in numpy in
// tests/voxel_map_ref.py, bit for bit.
//
// A record is (key, sum_q[3], count, obs): the 63-bit voxel key (21 index bits per axis, bias 2^20, x-major), the sums of the
// points' residuals inside the voxel in 2^-30 voxel units (int64), the number of points and the number of observations that
// put a point there.  The sums are integers, so fusing is associative and commutative: any batching, any order of insertion
// and any order of the run reduction give the same bits.  There is no floating-point atomic in this file; the 64-bit integer
// atomicAdd (a vector atomic) carries the runs that leave a wave.
//
// integrate   vm_offsets (one workgroup: sizes of the picked clouds, their scan, the point capacity), vm_key (world point, key,
//             residuals and observation of every point), radix_sort_pairs on the live count, vm_count / vm_scan / vm_head (run
//             heads by ballot + popcount; the head writes the key and zeroes its record), vm_reduce (a segmented scan inside
//             each wave; a run that lies inside one wave is stored, the pieces of any other run are added with integer atomics).
// merge       mg_search (every B row binary-searches A), mg_scan (B-only rows, the capacity decision), mg_rank (rank of every B
//             row among the B-only rows), mg_place_a / mg_place_b: pos(a_i) = i + |{B-only < a_i}|, pos(b_j) = rank(b_j) +
//             lower_bound_A(b_j), which for a matched row is its partner's position: it adds there.
// select      sel_slab (a box owns one contiguous key range: two binary searches on the x index), sel_count, sel_scan,
//             sel_write: the slab is cut into slices, each slice counts, then writes behind the scanned counts.
//
// No call synchronises with the host; grids are sized from capacities and the live counts stay on the device.
#include "../../include/egonn_hip.h"
#include "common.h"
#include "voxel_key.h"                                   // the frame, the key and the residuals of a point; shared with ndt.hip

#pragma clang fp contract(off)

namespace egonn {

static constexpr int VM_MAX_BOXES = 4096;
static constexpr int VM_MAX_SLICE_ROWS = 65536;          // slice counters of one select call

struct VmRec {                                           // struct-of-arrays view of records
  uint64_t* keys;
  int64_t* sums;                                         // (rows, 3)
  int32_t* count;
  int32_t* obs;
};
struct VmCRec {
  const uint64_t* keys;
  const int64_t* sums;
  const int32_t* count;
  const int32_t* obs;
};

__device__ static inline int64_t vm_min(int64_t a, int64_t b) { return a < b ? a : b; }

// one workgroup: exclusive scan of cnt[0..n) in place, the total to every thread
__device__ static inline int64_t vm_block_scan(int32_t* __restrict__ cnt, int64_t n, int64_t* s_sum) {
  const int t = threadIdx.x;
  const int64_t per = (n + VM_WG - 1) / VM_WG;
  const int64_t b0 = vm_min(t * per, n), b1 = vm_min(b0 + per, n);
  int64_t s = 0;
  for (int64_t b = b0; b < b1; ++b) s += cnt[b];
  s_sum[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t acc = 0;
    for (int k = 0; k < VM_WG; ++k) {
      const int64_t v = s_sum[k];
      s_sum[k] = acc;
      acc += v;
    }
    s_sum[VM_WG] = acc;
  }
  __syncthreads();
  int64_t acc = s_sum[t];
  for (int64_t b = b0; b < b1; ++b) {
    const int32_t v = cnt[b];
    cnt[b] = (int32_t)acc;
    acc += v;
  }
  return s_sum[VM_WG];
}

// ------------------------------------------------------------------ integrate
// vm_offsets_kernel (voxel_key.h): the picked clouds' offsets, BAD_INDEX, the point capacity
__global__ __launch_bounds__(VM_WG) void vm_key_kernel(const double* __restrict__ bank, int64_t n_bank, const int64_t* __restrict__ off,
                                                       int64_t n_clouds, const int32_t* __restrict__ pick,
                                                       const double* __restrict__ poses, int n_obs, VmFrame F,
                                                       const int64_t* __restrict__ obs_off, int64_t cap, uint64_t* __restrict__ keys,
                                                       uint32_t* __restrict__ vals, int4* __restrict__ q4, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * VM_WG + threadIdx.x;
  if (i >= clipi(obs_off[n_obs], cap)) return;
  int64_t src;
  const int k = vm_point_source(obs_off, n_obs, off, n_bank, n_clouds, pick, i, &src);
  uint64_t key = VM_INVALID;
  int4 q = make_int4(0, 0, 0, k);
  if (src >= 0) {
    int r[3];
    if (vm_point_key(bank + src * 3, poses + (int64_t)k * 16, F, &key, r)) q = make_int4(r[0], r[1], r[2], k);
  }
  if (key == VM_INVALID) atomicOr(status, EGONN_VMAP_STATUS_RANGE);
  keys[i] = key;
  vals[i] = (uint32_t)i;
  q4[i] = q;
}

__device__ static inline bool vm_is_head(const uint64_t* __restrict__ keys, int64_t n, int64_t i) {
  if (i >= n) return false;
  const uint64_t k = keys[i];
  return k != VM_INVALID && (i == 0 || keys[i - 1] != k);
}

__global__ __launch_bounds__(VM_WG) void vm_count_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ n_dev, int64_t cap,
                                                         int32_t* __restrict__ blockcnt) {
  __shared__ int s_w[4];
  const int t = threadIdx.x;
  const bool head = vm_is_head(keys, vm_live(n_dev, cap), (int64_t)blockIdx.x * VM_WG + t);
  const unsigned long long bal = __ballot(head);
  if ((t & 63) == 0) s_w[t >> 6] = __popcll(bal);
  __syncthreads();
  if (t == 0) blockcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// one workgroup: exclusive scan of the block counts, the number of voxels against the capacity.  meta[0] = 1: go on
__global__ __launch_bounds__(VM_WG) void vm_scan_kernel(int32_t* __restrict__ blockcnt, int64_t nb, int64_t capacity,
                                                        int64_t* __restrict__ n_out, int32_t* __restrict__ status,
                                                        int32_t* __restrict__ meta) {
  __shared__ int64_t s_sum[VM_WG + 1];
  const int64_t total = vm_block_scan(blockcnt, nb, s_sum);
  if (threadIdx.x == 0) {
    const bool fail = total > capacity;
    if (fail) atomicOr(status, EGONN_VMAP_STATUS_CAPACITY);
    *n_out = fail ? 0 : total;
    meta[0] = fail ? 0 : 1;
  }
}

// the run's first point writes the key and zeroes the record: vm_reduce adds into it
__global__ __launch_bounds__(VM_WG) void vm_head_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ n_dev, int64_t cap,
                                                        const int32_t* __restrict__ blockpre, const int32_t* __restrict__ meta, VmRec out,
                                                        int64_t capacity) {
  __shared__ int s_w[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t i = (int64_t)blockIdx.x * VM_WG + t;
  const bool head = meta[0] && vm_is_head(keys, vm_live(n_dev, cap), i);
  const unsigned long long bal = __ballot(head);
  if (lane == 0) s_w[w] = __popcll(bal);
  __syncthreads();
  if (!head) return;
  int64_t o = blockpre[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; ++k) o += s_w[k];
  if (o >= capacity) return;                  // cannot happen (vm_scan compared the total); keeps the stores in bounds regardless
  out.keys[o] = keys[i];
  out.sums[o * 3] = out.sums[o * 3 + 1] = out.sums[o * 3 + 2] = 0;
  out.count[o] = 0;
  out.obs[o] = 0;
}

__global__ __launch_bounds__(VM_WG) void vm_reduce_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                          const int4* __restrict__ q4, const int64_t* __restrict__ n_dev, int64_t cap,
                                                          const int32_t* __restrict__ blockpre, const int32_t* __restrict__ meta,
                                                          VmRec out, int64_t capacity) {
  __shared__ int s_w[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t i = (int64_t)blockIdx.x * VM_WG + t;
  const int64_t n = vm_live(n_dev, cap);
  const bool go = meta[0] != 0;
  const uint64_t key = i < n ? keys[i] : VM_INVALID;
  const bool valid = go && key != VM_INVALID;
  const bool head = valid && (i == 0 || keys[i - 1] != key);
  const unsigned long long bal = __ballot(head), vbal = __ballot(valid);
  if (lane == 0) s_w[w] = __popcll(bal);
  __syncthreads();
  if (vbal == 0ull) return;                                                 // a wave behind the last valid point
  const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);          // lanes <= this one
  int64_t o = (int64_t)blockpre[blockIdx.x] + __popcll(bal & upto) - 1;    // the record of this point's run
  for (int k = 0; k < w; ++k) o += s_w[k];
  int4 q = make_int4(0, 0, 0, -1);
  if (valid) {
    const uint32_t v = vals[i];
    if ((int64_t)v < cap) q = q4[v];
  }
  // observations of a run: the sort is stable and the points enter in observation order, so they are the changes of k
  int kprev = __shfl_up(q.w, 1);
  if (lane == 0 && valid && !head) {
    const uint32_t v = vals[i - 1];
    kprev = (int64_t)v < cap ? q4[v].w : -1;
  }
  long long sx = q.x, sy = q.y, sz = q.z;
  int cnt = valid ? 1 : 0, ob = valid && (head || kprev != q.w) ? 1 : 0;
  const unsigned long long hb = bal & upto;
  const int start = hb ? 63 - __clzll((long long)hb) : 0;                   // first lane of this point's run inside the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long ax = __shfl_up(sx, d), ay = __shfl_up(sy, d), az = __shfl_up(sz, d);
    const int ac = __shfl_up(cnt, d), ao = __shfl_up(ob, d);
    if (lane - d >= start) sx += ax, sy += ay, sz += az, cnt += ac, ob += ao;
  }
  // the last lane of a run's piece holds the piece's sums
  const bool next_valid = lane < 63 && ((vbal >> (lane + 1)) & 1ull), next_head = lane < 63 && ((bal >> (lane + 1)) & 1ull);
  if (!valid || (lane < 63 && next_valid && !next_head)) return;
  if (o < 0 || o >= capacity) return;                                       // cannot happen; keeps the stores in bounds regardless
  const bool begins_here = (bal >> start) & 1ull;
  const bool ends_here = i + 1 >= n || keys[i + 1] != key;
  if (begins_here && ends_here) {                                            // the whole run inside this wave: nobody else adds
    out.sums[o * 3] = sx, out.sums[o * 3 + 1] = sy, out.sums[o * 3 + 2] = sz;
    out.count[o] = cnt;
    out.obs[o] = ob;
  } else {
    unsigned long long* dst = (unsigned long long*)(out.sums + o * 3);
    atomicAdd(dst, (unsigned long long)sx);
    atomicAdd(dst + 1, (unsigned long long)sy);
    atomicAdd(dst + 2, (unsigned long long)sz);
    atomicAdd(out.count + o, cnt);
    atomicAdd(out.obs + o, ob);
  }
}

struct VmLayout {
  size_t obs_off, keys0, keys1, vals0, vals1, q4, blockcnt, meta, sort, sort_bytes, total;
  int64_t nb;
};
static VmLayout vm_layout(int64_t points_capacity, int n_obs) {
  VmLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
  const size_t m = (size_t)(points_capacity > 0 ? points_capacity : 1);
  L.nb = cdiv((int64_t)m, VM_WG);
  L.obs_off = take((size_t)(n_obs + 1) * 8);
  L.keys0 = take(m * 8), L.keys1 = take(m * 8), L.vals0 = take(m * 4), L.vals1 = take(m * 4);
  L.q4 = take(m * 16);
  L.blockcnt = take((size_t)(L.nb + 1) * 4);
  L.meta = take(256);
  // + 512: the sort carves two arrays out of this span and Arena::alloc aligns each carve to 256
  L.sort_bytes = align_up(radix_sort_scratch_bytes((int64_t)m) + 512, 256);
  L.sort = take(L.sort_bytes);
  L.total = o;
  return L;
}

// ------------------------------------------------------------------ merge
static constexpr uint32_t MG_MATCHED = 0x80000000u;

__global__ __launch_bounds__(VM_WG) void mg_search_kernel(const uint64_t* __restrict__ a_keys, const int64_t* __restrict__ n_a, int64_t cap_a,
                                                          const uint64_t* __restrict__ b_keys, const int64_t* __restrict__ n_b, int64_t cap_b,
                                                          uint32_t* __restrict__ lb_a, int32_t* __restrict__ blockcnt) {
  __shared__ int s_w[4];
  const int t = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * VM_WG + t;
  const int64_t na = vm_live(n_a, cap_a), nb = vm_live(n_b, cap_b);
  bool only = false;
  if (j < nb) {
    const uint64_t k = b_keys[j];
    const int64_t lb = vm_lower_bound(a_keys, na, k);
    const bool matched = lb < na && a_keys[lb] == k;
    lb_a[j] = (uint32_t)lb | (matched ? MG_MATCHED : 0u);
    only = !matched;
  }
  const unsigned long long bal = __ballot(only);
  if ((t & 63) == 0) s_w[t >> 6] = __popcll(bal);
  __syncthreads();
  if (t == 0) blockcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// meta[0] = 1: the union fits, meta[1] = B-only rows
__global__ __launch_bounds__(VM_WG) void mg_scan_kernel(int32_t* __restrict__ blockcnt, int64_t nblk, const int64_t* __restrict__ n_a,
                                                        int64_t cap_a, int64_t capacity_out, int64_t* __restrict__ n_out,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ meta) {
  __shared__ int64_t s_sum[VM_WG + 1];
  const int64_t only = vm_block_scan(blockcnt, nblk, s_sum);
  if (threadIdx.x == 0) {
    const int64_t na = vm_live(n_a, cap_a);
    const bool fail = na + only > capacity_out;
    if (fail) atomicOr(status, EGONN_VMAP_STATUS_CAPACITY);
    *n_out = fail ? na : na + only;
    meta[0] = fail ? 0 : 1;
    meta[1] = (int32_t)only;
  }
}

// rank[j] = B-only rows in front of row j, rank[n_b] = all of them
__global__ __launch_bounds__(VM_WG) void mg_rank_kernel(const uint32_t* __restrict__ lb_a, const int64_t* __restrict__ n_b, int64_t cap_b,
                                                        const int32_t* __restrict__ blockpre, const int32_t* __restrict__ meta,
                                                        int32_t* __restrict__ rank) {
  __shared__ int s_w[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t j = (int64_t)blockIdx.x * VM_WG + t;
  const int64_t nb = vm_live(n_b, cap_b);
  const bool only = j < nb && !(lb_a[j] & MG_MATCHED);
  const unsigned long long bal = __ballot(only);
  if (lane == 0) s_w[w] = __popcll(bal);
  __syncthreads();
  if (j > nb) return;
  if (j == nb) { rank[j] = meta[1]; return; }
  int r = blockpre[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; ++k) r += s_w[k];
  rank[j] = r;
}

__global__ __launch_bounds__(VM_WG) void mg_place_a_kernel(VmCRec A, const int64_t* __restrict__ n_a, int64_t cap_a,
                                                           const uint64_t* __restrict__ b_keys, const int64_t* __restrict__ n_b,
                                                           int64_t cap_b, const int32_t* __restrict__ rank, const int32_t* __restrict__ meta,
                                                           VmRec out, int64_t capacity_out) {
  const int64_t i = (int64_t)blockIdx.x * VM_WG + threadIdx.x;
  if (i >= vm_live(n_a, cap_a)) return;
  const uint64_t k = A.keys[i];
  const int64_t pos = meta[0] ? i + rank[vm_lower_bound(b_keys, vm_live(n_b, cap_b), k)] : i;      // the union does not fit: out = A
  if (pos >= capacity_out) return;            // cannot happen (mg_scan compared the total); keeps the stores in bounds regardless
  out.keys[pos] = k;
  out.sums[pos * 3] = A.sums[i * 3], out.sums[pos * 3 + 1] = A.sums[i * 3 + 1], out.sums[pos * 3 + 2] = A.sums[i * 3 + 2];
  out.count[pos] = A.count[i];
  out.obs[pos] = A.obs[i];
}

// after mg_place_a: a matched row adds into its partner's record (keys are unique: one B row per record, no atomic)
__global__ __launch_bounds__(VM_WG) void mg_place_b_kernel(VmCRec B, const int64_t* __restrict__ n_b, int64_t cap_b,
                                                           const uint32_t* __restrict__ lb_a, const int32_t* __restrict__ rank,
                                                           const int32_t* __restrict__ meta, VmRec out, int64_t capacity_out) {
  const int64_t j = (int64_t)blockIdx.x * VM_WG + threadIdx.x;
  if (!meta[0] || j >= vm_live(n_b, cap_b)) return;
  const uint32_t e = lb_a[j];
  const int64_t pos = (int64_t)(e & ~MG_MATCHED) + rank[j];
  if (pos >= capacity_out) return;
  if (e & MG_MATCHED) {
    out.sums[pos * 3] += B.sums[j * 3], out.sums[pos * 3 + 1] += B.sums[j * 3 + 1], out.sums[pos * 3 + 2] += B.sums[j * 3 + 2];
    out.count[pos] += B.count[j];
    out.obs[pos] += B.obs[j];
  } else {
    out.keys[pos] = B.keys[j];
    out.sums[pos * 3] = B.sums[j * 3], out.sums[pos * 3 + 1] = B.sums[j * 3 + 1], out.sums[pos * 3 + 2] = B.sums[j * 3 + 2];
    out.count[pos] = B.count[j];
    out.obs[pos] = B.obs[j];
  }
}

struct MgLayout {
  size_t lb_a, rank, blockcnt, meta, total;
  int64_t nblk;
};
static MgLayout mg_layout(int64_t capacity_b) {
  MgLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
  const size_t m = (size_t)(capacity_b > 0 ? capacity_b : 1);
  L.nblk = cdiv((int64_t)m, VM_WG);
  L.lb_a = take(m * 4);
  L.rank = take((m + 1) * 4);
  L.blockcnt = take((size_t)(L.nblk + 1) * 4);
  L.meta = take(256);
  L.total = o;
  return L;
}
static bool mg_shape_ok(int64_t capacity_a, int64_t capacity_b, int64_t capacity_out) {
  return capacity_a >= 0 && capacity_b >= 0 && capacity_a < (1ll << 31) && capacity_b < (1ll << 31) && capacity_out >= capacity_a &&
         capacity_out < (1ll << 31);
}

// ------------------------------------------------------------------ select
struct SelRule { int32_t min_count, min_obs; int relative; };

// the centroid of record i, and whether box b (centre, half extents; null = everywhere) takes it
__device__ static inline bool sel_take(const VmCRec& M, int64_t i, const VmFrame& F, const SelRule& R, const double* __restrict__ box,
                                       double* c) {
  const int32_t cnt = M.count[i];
  if (cnt < R.min_count || M.obs[i] < R.min_obs || cnt <= 0) return false;
  const uint64_t key = M.keys[i];
  const double den = (double)cnt * (double)VM_ONE;
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int64_t idx = (int64_t)((key >> ((2 - a) * VM_BITS)) & VM_MASK) - VM_BIAS;
    c[a] = ((double)idx + (double)M.sums[i * 3 + a] / den) * F.voxel + F.org[a];
    if (box) in = in && box[a] - box[3 + a] <= c[a] && c[a] < box[a] + box[3 + a];
  }
  return in;
}

// the contiguous key range of every box: the voxels whose x index can hold a centroid inside it
__global__ __launch_bounds__(VM_WG) void sel_slab_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ n_dev, int64_t cap,
                                                         VmFrame F, const double* __restrict__ boxes, int n_seg,
                                                         int64_t* __restrict__ slab) {
  const int b = blockIdx.x * VM_WG + threadIdx.x;
  if (b >= n_seg) return;
  const int64_t n = vm_live(n_dev, cap);
  int64_t lo = 0, hi = n;
  if (boxes) {
    const double cx = boxes[b * 6], hx = boxes[b * 6 + 3];
    // one voxel of margin on both sides: the exact test is sel_take's
    const double f0 = floor((cx - hx - F.org[0]) / F.voxel) - 1.0, f1 = floor((cx + hx - F.org[0]) / F.voxel) + 1.0;
    if (!(f0 <= f1)) {                                                      // NaN, or a negative half extent
      lo = hi = 0;
    } else {
      const double m = (double)VM_BIAS;
      const int64_t i0 = (int64_t)fmin(fmax(f0, -m), m), i1 = (int64_t)fmin(fmax(f1, -m - 1.0), m - 1.0);      // [i0, i1]
      lo = vm_lower_bound(keys, n, (uint64_t)(i0 + VM_BIAS) << (2 * VM_BITS));
      hi = vm_lower_bound(keys, n, (uint64_t)(i1 + 1 + VM_BIAS) << (2 * VM_BITS));
      if (hi < lo) hi = lo;
    }
  }
  slab[b * 2] = lo;
  slab[b * 2 + 1] = hi;
}

__device__ static inline void sel_slice(const int64_t* __restrict__ slab, int b, int s, int S, int64_t* a, int64_t* e) {
  const int64_t lo = slab[b * 2], len = slab[b * 2 + 1] - lo;
  const int64_t per = (len + S - 1) / S;
  *a = lo + vm_min(s * per, len);
  *e = lo + vm_min((s + 1) * per, len);
}

__global__ __launch_bounds__(VM_WG) void sel_count_kernel(VmCRec M, VmFrame F, SelRule R, const double* __restrict__ boxes,
                                                          const int64_t* __restrict__ slab, int S, int32_t* __restrict__ cnts) {
  __shared__ int s_w[4];
  const int s = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  int64_t a, e;
  sel_slice(slab, b, s, S, &a, &e);
  const double* box = boxes ? boxes + (int64_t)b * 6 : nullptr;
  int mine = 0;
  double c[3];
  for (int64_t i = a + t; i < e; i += VM_WG) mine += sel_take(M, i, F, R, box, c) ? 1 : 0;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
  if ((t & 63) == 0) s_w[t >> 6] = mine;
  __syncthreads();
  if (t == 0) cnts[(int64_t)b * S + s] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// meta[0] = 1: write.  sizing (no out_points): the offsets only
__global__ __launch_bounds__(VM_WG) void sel_scan_kernel(int32_t* __restrict__ cnts, int n_seg, int S, int64_t capacity, int sizing,
                                                         int64_t* __restrict__ out_offsets, int32_t* __restrict__ status,
                                                         int32_t* __restrict__ meta) {
  __shared__ int64_t s_sum[VM_WG + 1];
  __shared__ int s_fail;
  const int64_t total = vm_block_scan(cnts, (int64_t)n_seg * S, s_sum);
  if (threadIdx.x == 0) {
    s_fail = total > (sizing ? (int64_t)INT32_MAX : capacity);      // sizing: the offsets must fit the int32 scan
    if (s_fail) atomicOr(status, EGONN_VMAP_STATUS_CAPACITY);
    meta[0] = s_fail ? 0 : 1;
    out_offsets[n_seg] = s_fail ? 0 : total;
  }
  __threadfence_block();
  __syncthreads();
  for (int b = threadIdx.x; b < n_seg; b += VM_WG) out_offsets[b] = s_fail ? 0 : cnts[(int64_t)b * S];
}

__global__ __launch_bounds__(VM_WG) void sel_write_kernel(VmCRec M, VmFrame F, SelRule R, const double* __restrict__ boxes,
                                                          const int64_t* __restrict__ slab, int S, const int32_t* __restrict__ pre,
                                                          const int32_t* __restrict__ meta, double* __restrict__ out_points,
                                                          int32_t* __restrict__ out_count, int32_t* __restrict__ out_obs,
                                                          int64_t capacity) {
  __shared__ int s_w[4];
  if (!meta[0]) return;
  const int s = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
  int64_t a, e;
  sel_slice(slab, b, s, S, &a, &e);
  const double* box = boxes ? boxes + (int64_t)b * 6 : nullptr;
  int64_t base = pre[(int64_t)b * S + s];
  for (int64_t i0 = a; i0 < e; i0 += VM_WG) {                               // uniform trip count: every thread meets the barriers
    const int64_t i = i0 + t;
    double c[3] = {0.0, 0.0, 0.0};
    const bool take = i < e && sel_take(M, i, F, R, box, c);
    const unsigned long long bal = __ballot(take);
    __syncthreads();                                                        // the previous tile's s_w has been read
    if (lane == 0) s_w[w] = __popcll(bal);
    __syncthreads();
    if (take) {
      int64_t o = base + __popcll(bal & ((1ull << lane) - 1ull));
      for (int k = 0; k < w; ++k) o += s_w[k];
      if (o < capacity) {                                                   // always (sel_scan compared the total)
#pragma unroll
        for (int k = 0; k < 3; ++k) out_points[o * 3 + k] = R.relative && box ? c[k] - box[k] : c[k];
        if (out_count) out_count[o] = M.count[i];
        if (out_obs) out_obs[o] = M.obs[i];
      }
    }
    base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
  }
}

struct SelLayout {
  size_t slab, cnts, meta, total;
  int n_seg, S;
};
static SelLayout sel_layout(int64_t capacity_map, int n_boxes) {
  SelLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
  L.n_seg = n_boxes > 0 ? n_boxes : 1;
  int64_t S = cdiv(capacity_map > 0 ? capacity_map : 1, 2048);            // slices per box: about 2048 records each at a full slab
  const int64_t most = VM_MAX_SLICE_ROWS / L.n_seg;
  S = S > most ? most : S;
  L.S = (int)(S < 1 ? 1 : (S > 1024 ? 1024 : S));
  L.slab = take((size_t)L.n_seg * 16);
  L.cnts = take(((size_t)L.n_seg * L.S + 1) * 4);
  L.meta = take(256);
  L.total = o;
  return L;
}
static bool sel_shape_ok(int64_t capacity_map, int n_boxes) {
  return capacity_map >= 0 && capacity_map < (1ll << 31) && n_boxes >= 0 && n_boxes <= VM_MAX_BOXES;
}

}  // namespace egonn

using namespace egonn;

// ------------------------------------------------------------------ entry points
API int64_t egonn_voxel_map_integrate_scratch_bytes(int64_t points_capacity, int n_obs) {
  if (!vm_integrate_shape_ok(points_capacity, n_obs)) return -1;
  return (int64_t)vm_layout(points_capacity, n_obs).total;
}

API int egonn_voxel_map_integrate(const double* bank, int64_t n_bank, const int64_t* bank_offsets, int64_t n_clouds, const int32_t* pick,
                                  const double* poses, int n_obs, const double* origin, double voxel, int64_t points_capacity,
                                  uint64_t* out_keys, int64_t* out_sums, int32_t* out_count, int32_t* out_obs, int64_t capacity,
                                  int64_t* n_out, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(n_bank >= 0 && n_clouds >= 0 && n_clouds < (1ll << 31) && vm_integrate_shape_ok(points_capacity, n_obs) &&
                    capacity >= 0 && capacity < (1ll << 31),
                EGONN_ERR_INVALID, "voxel_map_integrate: bad shape (n_bank=%lld, n_clouds=%lld, n_obs=%d in [1, %d], "
                "points_capacity=%lld, capacity=%lld; both < 2^31)", (long long)n_bank, (long long)n_clouds, n_obs, VM_MAX_OBS,
                (long long)points_capacity, (long long)capacity);
  EGONN_REQUIRE(vm_frame_ok(origin, voxel), EGONN_ERR_INVALID, "voxel_map_integrate: voxel must be finite and > 0, origin finite");
  EGONN_REQUIRE(bank_offsets && pick && poses && n_out && status && scratch && (n_bank == 0 || bank) &&
                    (capacity == 0 || (out_keys && out_sums && out_count && out_obs)),
                EGONN_ERR_INVALID, "voxel_map_integrate: null pointer");
  const VmLayout L = vm_layout(points_capacity, n_obs);
  EGONN_REQUIRE(scratch_bytes >= (int64_t)L.total && ((uintptr_t)scratch & 255) == 0, EGONN_ERR_INVALID,
                "voxel_map_integrate: scratch needs %lld bytes, 256-byte aligned", (long long)L.total);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)scratch;
  int64_t* obs_off = (int64_t*)(base + L.obs_off);
  uint64_t *k0 = (uint64_t*)(base + L.keys0), *k1 = (uint64_t*)(base + L.keys1);
  uint32_t *v0 = (uint32_t*)(base + L.vals0), *v1 = (uint32_t*)(base + L.vals1);
  int4* q4 = (int4*)(base + L.q4);
  int32_t* blockcnt = (int32_t*)(base + L.blockcnt);
  int32_t* meta = (int32_t*)(base + L.meta);
  VmFrame F = {{origin[0], origin[1], origin[2]}, voxel};
  const VmRec out = {out_keys, out_sums, out_count, out_obs};
  const dim3 grid((unsigned)L.nb), wg(VM_WG);
  const int64_t* total = obs_off + n_obs;
  hipLaunchKernelGGL(vm_offsets_kernel, dim3(1), wg, 0, st, bank_offsets, n_bank, n_clouds, pick, n_obs, points_capacity, obs_off,
                     status);
  hipLaunchKernelGGL(vm_key_kernel, grid, wg, 0, st, bank, n_bank, bank_offsets, n_clouds, pick, poses, n_obs, F, obs_off,
                     points_capacity, k0, v0, q4, status);
  uint64_t* keys = k0;
  uint32_t* vals = v0;
  if (points_capacity > 0) {
    Arena sort_ws = Arena::view(base + L.sort, L.sort_bytes);
    EGONN_TRY(radix_sort_pairs(sort_ws, k0, v0, k1, v1, points_capacity, 64, st, total, &keys, &vals));
  }
  hipLaunchKernelGGL(vm_count_kernel, grid, wg, 0, st, keys, total, points_capacity, blockcnt);
  hipLaunchKernelGGL(vm_scan_kernel, dim3(1), wg, 0, st, blockcnt, L.nb, capacity, n_out, status, meta);
  hipLaunchKernelGGL(vm_head_kernel, grid, wg, 0, st, keys, total, points_capacity, blockcnt, meta, out, capacity);
  hipLaunchKernelGGL(vm_reduce_kernel, grid, wg, 0, st, keys, vals, q4, total, points_capacity, blockcnt, meta, out, capacity);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int64_t egonn_voxel_map_merge_scratch_bytes(int64_t capacity_a, int64_t capacity_b, int64_t capacity_out) {
  if (!mg_shape_ok(capacity_a, capacity_b, capacity_out)) return -1;
  return (int64_t)mg_layout(capacity_b).total;
}

API int egonn_voxel_map_merge(const uint64_t* a_keys, const int64_t* a_sums, const int32_t* a_count, const int32_t* a_obs,
                              const int64_t* n_a, int64_t capacity_a, const uint64_t* b_keys, const int64_t* b_sums,
                              const int32_t* b_count, const int32_t* b_obs, const int64_t* n_b, int64_t capacity_b, uint64_t* out_keys,
                              int64_t* out_sums, int32_t* out_count, int32_t* out_obs, int64_t capacity_out, int64_t* n_out,
                              int32_t* status, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(mg_shape_ok(capacity_a, capacity_b, capacity_out), EGONN_ERR_INVALID,
                "voxel_map_merge: bad shape (capacity_a=%lld, capacity_b=%lld, capacity_out=%lld >= capacity_a; all < 2^31)",
                (long long)capacity_a, (long long)capacity_b, (long long)capacity_out);
  EGONN_REQUIRE(n_a && n_b && n_out && status && scratch && (capacity_a == 0 || (a_keys && a_sums && a_count && a_obs)) &&
                    (capacity_b == 0 || (b_keys && b_sums && b_count && b_obs)) &&
                    (capacity_out == 0 || (out_keys && out_sums && out_count && out_obs)),
                EGONN_ERR_INVALID, "voxel_map_merge: null pointer");
  EGONN_REQUIRE(capacity_out == 0 || (out_keys != a_keys && out_keys != b_keys), EGONN_ERR_INVALID,
                "voxel_map_merge: out must not be A or B");
  const MgLayout L = mg_layout(capacity_b);
  EGONN_REQUIRE(scratch_bytes >= (int64_t)L.total && ((uintptr_t)scratch & 255) == 0, EGONN_ERR_INVALID,
                "voxel_map_merge: scratch needs %lld bytes, 256-byte aligned", (long long)L.total);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)scratch;
  uint32_t* lb_a = (uint32_t*)(base + L.lb_a);
  int32_t* rank = (int32_t*)(base + L.rank);
  int32_t* blockcnt = (int32_t*)(base + L.blockcnt);
  int32_t* meta = (int32_t*)(base + L.meta);
  const VmCRec A = {a_keys, a_sums, a_count, a_obs}, B = {b_keys, b_sums, b_count, b_obs};
  const VmRec out = {out_keys, out_sums, out_count, out_obs};
  const dim3 wg(VM_WG), grid_b((unsigned)L.nblk);
  hipLaunchKernelGGL(mg_search_kernel, grid_b, wg, 0, st, a_keys, n_a, capacity_a, b_keys, n_b, capacity_b, lb_a, blockcnt);
  hipLaunchKernelGGL(mg_scan_kernel, dim3(1), wg, 0, st, blockcnt, L.nblk, n_a, capacity_a, capacity_out, n_out, status, meta);
  hipLaunchKernelGGL(mg_rank_kernel, dim3((unsigned)cdiv(capacity_b + 1, VM_WG)), wg, 0, st, lb_a, n_b, capacity_b, blockcnt, meta, rank);
  if (capacity_a > 0)
    hipLaunchKernelGGL(mg_place_a_kernel, dim3((unsigned)cdiv(capacity_a, VM_WG)), wg, 0, st, A, n_a, capacity_a, b_keys, n_b, capacity_b,
                       rank, meta, out, capacity_out);
  if (capacity_b > 0)
    hipLaunchKernelGGL(mg_place_b_kernel, grid_b, wg, 0, st, B, n_b, capacity_b, lb_a, rank, meta, out, capacity_out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int64_t egonn_voxel_map_select_scratch_bytes(int64_t capacity_map, int n_boxes) {
  if (!sel_shape_ok(capacity_map, n_boxes)) return -1;
  return (int64_t)sel_layout(capacity_map, n_boxes).total;
}

API int egonn_voxel_map_select(const uint64_t* keys, const int64_t* sums, const int32_t* count, const int32_t* obs, const int64_t* n_dev,
                               int64_t capacity_map, const double* origin, double voxel, int min_count, int min_obs,
                               const double* boxes, int n_boxes, int relative, double* out_points, int64_t* out_offsets,
                               int32_t* out_count, int32_t* out_obs, int64_t capacity, int32_t* status, void* scratch,
                               int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(sel_shape_ok(capacity_map, n_boxes) && capacity >= 0 && capacity < (1ll << 31), EGONN_ERR_INVALID,
                "voxel_map_select: bad shape (capacity_map=%lld, n_boxes=%d in [0, %d], capacity=%lld; both < 2^31)",
                (long long)capacity_map, n_boxes, VM_MAX_BOXES, (long long)capacity);
  EGONN_REQUIRE(vm_frame_ok(origin, voxel), EGONN_ERR_INVALID, "voxel_map_select: voxel must be finite and > 0, origin finite");
  EGONN_REQUIRE(min_count >= 0 && min_obs >= 0, EGONN_ERR_INVALID, "voxel_map_select: negative min_count or min_obs");
  EGONN_REQUIRE((boxes != nullptr) == (n_boxes > 0), EGONN_ERR_INVALID, "voxel_map_select: boxes and n_boxes disagree");
  EGONN_REQUIRE(!relative || boxes, EGONN_ERR_INVALID, "voxel_map_select: relative needs boxes");
  EGONN_REQUIRE(n_dev && out_offsets && status && scratch && (capacity_map == 0 || (keys && sums && count && obs)) &&
                    (out_points || (!out_count && !out_obs)),
                EGONN_ERR_INVALID, "voxel_map_select: null pointer");
  const SelLayout L = sel_layout(capacity_map, n_boxes);
  EGONN_REQUIRE(scratch_bytes >= (int64_t)L.total && ((uintptr_t)scratch & 255) == 0, EGONN_ERR_INVALID,
                "voxel_map_select: scratch needs %lld bytes, 256-byte aligned", (long long)L.total);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)scratch;
  int64_t* slab = (int64_t*)(base + L.slab);
  int32_t* cnts = (int32_t*)(base + L.cnts);
  int32_t* meta = (int32_t*)(base + L.meta);
  VmFrame F = {{origin[0], origin[1], origin[2]}, voxel};
  const SelRule R = {min_count, min_obs, relative ? 1 : 0};
  const VmCRec M = {keys, sums, count, obs};
  const dim3 wg(VM_WG), grid((unsigned)L.S, (unsigned)L.n_seg);
  hipLaunchKernelGGL(sel_slab_kernel, dim3((unsigned)cdiv(L.n_seg, VM_WG)), wg, 0, st, keys, n_dev, capacity_map, F, boxes, L.n_seg, slab);
  hipLaunchKernelGGL(sel_count_kernel, grid, wg, 0, st, M, F, R, boxes, slab, L.S, cnts);
  hipLaunchKernelGGL(sel_scan_kernel, dim3(1), wg, 0, st, cnts, L.n_seg, L.S, capacity, out_points ? 0 : 1, out_offsets, status, meta);
  if (out_points)
    hipLaunchKernelGGL(sel_write_kernel, grid, wg, 0, st, M, F, R, boxes, slab, L.S, cnts, meta, out_points, out_count, out_obs, capacity);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
