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
// Counting flags per workgroup, scanning the counts in one workgroup, ranking a flagged row and the bounds of a run inside a
// wave are compact.h (wg_count, wg_scan, wg_rank, wave_run); what a head is stays here (vm_is_head).  The carves of a caller's
// scratch are one function per entry point (vm_span, mg_span, sel_span) over common.h's Carve.
//
// No call synchronises with the host; grids are sized from capacities and the live counts stay on the device.
#include "../../include/egonn_hip.h"
#include "common.h"
#include "compact.h"                                     // wg_count / wg_scan / wg_rank, wave_run
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
  const int heads = wg_count<VM_WG>(vm_is_head(keys, vm_live(n_dev, cap), (int64_t)blockIdx.x * VM_WG + threadIdx.x));
  if (threadIdx.x == 0) blockcnt[blockIdx.x] = heads;
}

// one workgroup: exclusive scan of the block counts, the number of voxels against the capacity.  meta[0] = 1: go on
__global__ __launch_bounds__(VM_WG) void vm_scan_kernel(int32_t* __restrict__ blockcnt, int64_t nb, int64_t capacity,
                                                        int64_t* __restrict__ n_out, int32_t* __restrict__ status,
                                                        int32_t* __restrict__ meta) {
  const int64_t total = wg_scan<VM_WG>(blockcnt, nb);
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
  const int64_t i = (int64_t)blockIdx.x * VM_WG + threadIdx.x;
  const bool head = meta[0] && vm_is_head(keys, vm_live(n_dev, cap), i);
  const int64_t o = (int64_t)blockpre[blockIdx.x] + wg_rank<VM_WG>(__ballot(head));
  if (!head) return;
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
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * VM_WG + threadIdx.x;
  const int64_t n = vm_live(n_dev, cap);
  const bool go = meta[0] != 0;
  const uint64_t key = i < n ? keys[i] : VM_INVALID;
  const bool valid = go && key != VM_INVALID;
  const bool head = valid && (i == 0 || keys[i - 1] != key);
  const unsigned long long bal = __ballot(head), vbal = __ballot(valid);
  const int64_t o = (int64_t)blockpre[blockIdx.x] + wg_rank<VM_WG>(bal) + (head ? 1 : 0) - 1;       // the record of this point's run
  if (vbal == 0ull) return;                                                 // a wave behind the last valid point
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
  const WaveRun run = wave_run(bal);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long ax = __shfl_up(sx, d), ay = __shfl_up(sy, d), az = __shfl_up(sz, d);
    const int ac = __shfl_up(cnt, d), ao = __shfl_up(ob, d);
    if (lane - d >= run.start) sx += ax, sy += ay, sz += az, cnt += ac, ob += ao;
  }
  // the last lane of a run's piece holds the piece's sums
  const bool next_valid = lane < 63 && ((vbal >> (lane + 1)) & 1ull), next_head = lane < 63 && ((bal >> (lane + 1)) & 1ull);
  if (!valid || (lane < 63 && next_valid && !next_head)) return;
  if (o < 0 || o >= capacity) return;                                       // cannot happen; keeps the stores in bounds regardless
  const bool ends_here = i + 1 >= n || keys[i + 1] != key;
  if (run.begins_here && ends_here) {                                        // the whole run inside this wave: nobody else adds
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

// The carves of the caller's scratch, one function per entry point.  With scratch = nullptr only `total` means anything
struct VmSpan {
  int64_t nb;               // workgroups over the points
  int64_t* obs_off;
  uint64_t* keys[2];        // ping-pong buffers of the sort
  uint32_t* vals[2];
  int4* q4;
  int32_t *blockcnt, *meta;
  Arena sort_ws;
  size_t total;
};
static VmSpan vm_span(void* scratch, int64_t points_capacity, int n_obs) {
  VmSpan S;
  Carve c(scratch);
  const size_t m = (size_t)(points_capacity > 0 ? points_capacity : 1);
  S.nb = cdiv((int64_t)m, VM_WG);
  S.obs_off = c.take<int64_t>((size_t)n_obs + 1);
  for (int k = 0; k < 2; ++k) S.keys[k] = c.take<uint64_t>(m);
  for (int k = 0; k < 2; ++k) S.vals[k] = c.take<uint32_t>(m);
  S.q4 = c.take<int4>(m);
  S.blockcnt = c.take<int32_t>((size_t)S.nb + 1);
  S.meta = c.take<int32_t>(64);
  S.sort_ws = c.sort_arena(radix_sort_scratch_bytes((int64_t)m));
  S.total = c.total();
  return S;
}

// ------------------------------------------------------------------ merge
static constexpr uint32_t MG_MATCHED = 0x80000000u;

__global__ __launch_bounds__(VM_WG) void mg_search_kernel(const uint64_t* __restrict__ a_keys, const int64_t* __restrict__ n_a, int64_t cap_a,
                                                          const uint64_t* __restrict__ b_keys, const int64_t* __restrict__ n_b, int64_t cap_b,
                                                          uint32_t* __restrict__ lb_a, int32_t* __restrict__ blockcnt) {
  const int64_t j = (int64_t)blockIdx.x * VM_WG + threadIdx.x;
  const int64_t na = vm_live(n_a, cap_a), nb = vm_live(n_b, cap_b);
  bool only = false;
  if (j < nb) {
    const uint64_t k = b_keys[j];
    const int64_t lb = vm_lower_bound(a_keys, na, k);
    const bool matched = lb < na && a_keys[lb] == k;
    lb_a[j] = (uint32_t)lb | (matched ? MG_MATCHED : 0u);
    only = !matched;
  }
  const int onlys = wg_count<VM_WG>(only);
  if (threadIdx.x == 0) blockcnt[blockIdx.x] = onlys;
}

// meta[0] = 1: the union fits, meta[1] = B-only rows
__global__ __launch_bounds__(VM_WG) void mg_scan_kernel(int32_t* __restrict__ blockcnt, int64_t nblk, const int64_t* __restrict__ n_a,
                                                        int64_t cap_a, int64_t capacity_out, int64_t* __restrict__ n_out,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ meta) {
  const int64_t only = wg_scan<VM_WG>(blockcnt, nblk);
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
  const int64_t j = (int64_t)blockIdx.x * VM_WG + threadIdx.x;
  const int64_t nb = vm_live(n_b, cap_b);
  const bool only = j < nb && !(lb_a[j] & MG_MATCHED);
  const int r = blockpre[blockIdx.x] + wg_rank<VM_WG>(__ballot(only));
  if (j > nb) return;
  rank[j] = j == nb ? meta[1] : r;
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

struct MgSpan {
  int64_t nblk;             // workgroups over the B rows
  uint32_t* lb_a;
  int32_t *rank, *blockcnt, *meta;
  size_t total;
};
static MgSpan mg_span(void* scratch, int64_t capacity_b) {
  MgSpan S;
  Carve c(scratch);
  const size_t m = (size_t)(capacity_b > 0 ? capacity_b : 1);
  S.nblk = cdiv((int64_t)m, VM_WG);
  S.lb_a = c.take<uint32_t>(m);
  S.rank = c.take<int32_t>(m + 1);
  S.blockcnt = c.take<int32_t>((size_t)S.nblk + 1);
  S.meta = c.take<int32_t>(64);
  S.total = c.total();
  return S;
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
  const int s = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  int64_t a, e;
  sel_slice(slab, b, s, S, &a, &e);
  const double* box = boxes ? boxes + (int64_t)b * 6 : nullptr;
  int mine = 0;
  double c[3];
  for (int64_t i = a + t; i < e; i += VM_WG) mine += sel_take(M, i, F, R, box, c) ? 1 : 0;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
  const int taken = wg_wave_sum<VM_WG>(mine);                                // lane 0 holds its wave's sum
  if (t == 0) cnts[(int64_t)b * S + s] = taken;
}

// meta[0] = 1: write.  sizing (no out_points): the offsets only
__global__ __launch_bounds__(VM_WG) void sel_scan_kernel(int32_t* __restrict__ cnts, int n_seg, int S, int64_t capacity, int sizing,
                                                         int64_t* __restrict__ out_offsets, int32_t* __restrict__ status,
                                                         int32_t* __restrict__ meta) {
  __shared__ int s_fail;
  const int64_t total = wg_scan<VM_WG>(cnts, (int64_t)n_seg * S);
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
  if (!meta[0]) return;
  const int s = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  int64_t a, e;
  sel_slice(slab, b, s, S, &a, &e);
  const double* box = boxes ? boxes + (int64_t)b * 6 : nullptr;
  int64_t base = pre[(int64_t)b * S + s];
  for (int64_t i0 = a; i0 < e; i0 += VM_WG) {                               // uniform trip count: every thread meets the barriers
    const int64_t i = i0 + t;
    double c[3] = {0.0, 0.0, 0.0};
    const bool take = i < e && sel_take(M, i, F, R, box, c);
    int taken;
    const int64_t o = base + wg_rank<VM_WG>(__ballot(take), &taken);
    if (take) {
      if (o < capacity) {                                                   // always (sel_scan compared the total)
#pragma unroll
        for (int k = 0; k < 3; ++k) out_points[o * 3 + k] = R.relative && box ? c[k] - box[k] : c[k];
        if (out_count) out_count[o] = M.count[i];
        if (out_obs) out_obs[o] = M.obs[i];
      }
    }
    base += taken;
  }
}

struct SelSpan {
  int n_seg, S;             // boxes (one without boxes), slices per box
  int64_t* slab;
  int32_t *cnts, *meta;
  size_t total;
};
static SelSpan sel_span(void* scratch, int64_t capacity_map, int n_boxes) {
  SelSpan L;
  Carve c(scratch);
  L.n_seg = n_boxes > 0 ? n_boxes : 1;
  int64_t S = cdiv(capacity_map > 0 ? capacity_map : 1, 2048);            // slices per box: about 2048 records each at a full slab
  const int64_t most = VM_MAX_SLICE_ROWS / L.n_seg;
  S = S > most ? most : S;
  L.S = (int)(S < 1 ? 1 : (S > 1024 ? 1024 : S));
  L.slab = c.take<int64_t>((size_t)L.n_seg * 2);
  L.cnts = c.take<int32_t>((size_t)L.n_seg * L.S + 1);
  L.meta = c.take<int32_t>(64);
  L.total = c.total();
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
  return (int64_t)vm_span(nullptr, points_capacity, n_obs).total;
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
  VmSpan S = vm_span(scratch, points_capacity, n_obs);
  EGONN_TRY(span_check("voxel_map_integrate", scratch, scratch_bytes, S.total));
  hipStream_t st = (hipStream_t)stream;
  VmFrame F = {{origin[0], origin[1], origin[2]}, voxel};
  const VmRec out = {out_keys, out_sums, out_count, out_obs};
  const dim3 grid((unsigned)S.nb), wg(VM_WG);
  const int64_t* total = S.obs_off + n_obs;
  hipLaunchKernelGGL(vm_offsets_kernel, dim3(1), wg, 0, st, bank_offsets, n_bank, n_clouds, pick, n_obs, points_capacity, S.obs_off,
                     status);
  hipLaunchKernelGGL(vm_key_kernel, grid, wg, 0, st, bank, n_bank, bank_offsets, n_clouds, pick, poses, n_obs, F, S.obs_off,
                     points_capacity, S.keys[0], S.vals[0], S.q4, status);
  uint64_t* keys = S.keys[0];
  uint32_t* vals = S.vals[0];
  if (points_capacity > 0)
    EGONN_TRY(radix_sort_pairs(S.sort_ws, S.keys[0], S.vals[0], S.keys[1], S.vals[1], points_capacity, 64, st, total, &keys, &vals));
  hipLaunchKernelGGL(vm_count_kernel, grid, wg, 0, st, keys, total, points_capacity, S.blockcnt);
  hipLaunchKernelGGL(vm_scan_kernel, dim3(1), wg, 0, st, S.blockcnt, S.nb, capacity, n_out, status, S.meta);
  hipLaunchKernelGGL(vm_head_kernel, grid, wg, 0, st, keys, total, points_capacity, S.blockcnt, S.meta, out, capacity);
  hipLaunchKernelGGL(vm_reduce_kernel, grid, wg, 0, st, keys, vals, S.q4, total, points_capacity, S.blockcnt, S.meta, out, capacity);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int64_t egonn_voxel_map_merge_scratch_bytes(int64_t capacity_a, int64_t capacity_b, int64_t capacity_out) {
  if (!mg_shape_ok(capacity_a, capacity_b, capacity_out)) return -1;
  return (int64_t)mg_span(nullptr, capacity_b).total;
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
  const MgSpan S = mg_span(scratch, capacity_b);
  EGONN_TRY(span_check("voxel_map_merge", scratch, scratch_bytes, S.total));
  hipStream_t st = (hipStream_t)stream;
  const VmCRec A = {a_keys, a_sums, a_count, a_obs}, B = {b_keys, b_sums, b_count, b_obs};
  const VmRec out = {out_keys, out_sums, out_count, out_obs};
  const dim3 wg(VM_WG), grid_b((unsigned)S.nblk);
  hipLaunchKernelGGL(mg_search_kernel, grid_b, wg, 0, st, a_keys, n_a, capacity_a, b_keys, n_b, capacity_b, S.lb_a, S.blockcnt);
  hipLaunchKernelGGL(mg_scan_kernel, dim3(1), wg, 0, st, S.blockcnt, S.nblk, n_a, capacity_a, capacity_out, n_out, status, S.meta);
  hipLaunchKernelGGL(mg_rank_kernel, dim3((unsigned)cdiv(capacity_b + 1, VM_WG)), wg, 0, st, S.lb_a, n_b, capacity_b, S.blockcnt, S.meta,
                     S.rank);
  if (capacity_a > 0)
    hipLaunchKernelGGL(mg_place_a_kernel, dim3((unsigned)cdiv(capacity_a, VM_WG)), wg, 0, st, A, n_a, capacity_a, b_keys, n_b, capacity_b,
                       S.rank, S.meta, out, capacity_out);
  if (capacity_b > 0)
    hipLaunchKernelGGL(mg_place_b_kernel, grid_b, wg, 0, st, B, n_b, capacity_b, S.lb_a, S.rank, S.meta, out, capacity_out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int64_t egonn_voxel_map_select_scratch_bytes(int64_t capacity_map, int n_boxes) {
  if (!sel_shape_ok(capacity_map, n_boxes)) return -1;
  return (int64_t)sel_span(nullptr, capacity_map, n_boxes).total;
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
  const SelSpan L = sel_span(scratch, capacity_map, n_boxes);
  EGONN_TRY(span_check("voxel_map_select", scratch, scratch_bytes, L.total));
  hipStream_t st = (hipStream_t)stream;
  VmFrame F = {{origin[0], origin[1], origin[2]}, voxel};
  const SelRule R = {min_count, min_obs, relative ? 1 : 0};
  const VmCRec M = {keys, sums, count, obs};
  const dim3 wg(VM_WG), grid((unsigned)L.S, (unsigned)L.n_seg);
  hipLaunchKernelGGL(sel_slab_kernel, dim3((unsigned)cdiv(L.n_seg, VM_WG)), wg, 0, st, keys, n_dev, capacity_map, F, boxes, L.n_seg,
                     L.slab);
  hipLaunchKernelGGL(sel_count_kernel, grid, wg, 0, st, M, F, R, boxes, L.slab, L.S, L.cnts);
  hipLaunchKernelGGL(sel_scan_kernel, dim3(1), wg, 0, st, L.cnts, L.n_seg, L.S, capacity, out_points ? 0 : 1, out_offsets, status,
                     L.meta);
  if (out_points)
    hipLaunchKernelGGL(sel_write_kernel, grid, wg, 0, st, M, F, R, boxes, L.slab, L.S, L.cnts, L.meta, out_points, out_count, out_obs,
                       capacity);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
