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
// subtract    sb_flag (every A row binary-searches B, forms r = A - B and flags keep / matched / illegal; three counts per
//             workgroup), sb_scan (one workgroup: n_out and the verdict), sb_write (rows placed with wg_rank; MISMATCH: out = A).
// moments     a map may carry the NDT layer's integer moments s1 / s2 per voxel (`*_moments`, subtract): the head, reduce and
//             placement kernels are templates on MOMENTS and the plain entry points are their <false> instances.
// select      sel_slab (a box owns one contiguous key range: two binary searches on the x index), sel_count, sel_scan,
//             sel_write: the slab is cut into slices, each slice counts, then writes behind the scanned counts.
//
// Counting flags per workgroup, scanning the counts in one workgroup, ranking a flagged row and the bounds of a run inside a
// wave are compact.h (wg_count, wg_scan, wg_rank, wave_run); what a head is stays here (vm_is_head).  The carves of a caller's
// scratch are one function per entry point (vm_span, mg_span, sb_span, sel_span) over common.h's Carve.
//
// No call synchronises with the host; grids are sized from capacities and the live counts stay on the device.
#include "../../include/egonn_hip.h"
#include "common.h"
#include "compact.h"                                     // wg_count / wg_scan / wg_rank, wave_run
#include "voxel_key.h"                                   // the frame, the key and the residuals of a point; shared with ndt.hip
#include <initializer_list>

#pragma clang fp contract(off)

namespace egonn {

static constexpr int VM_MAX_BOXES = 4096;
static constexpr int VM_MAX_SLICE_ROWS = 65536;          // slice counters of one select call

struct VmRec {                                           // struct-of-arrays view of records
  uint64_t* keys;
  int64_t* sums;                                         // (rows, 3)
  int32_t* count;
  int32_t* obs;
  int64_t* s1;                                           // (rows, 3), (rows, 6): the NDT moments, null without them
  int64_t* s2;
};
struct VmCRec {
  const uint64_t* keys;
  const int64_t* sums;
  const int32_t* count;
  const int32_t* obs;
  const int64_t* s1;
  const int64_t* s2;
};
static constexpr int VM_MOMENT_SHIFT = 10;               // m = q >> 10, the NDT layer's moments (ndt.hip: NDT_MOMENT_SHIFT)

// all given or all null, over every operand of a call
static inline bool vm_moments_agree(std::initializer_list<const void*> p, bool* given) {
  int set = 0;
  for (const void* q : p) set += q != nullptr;
  *given = set != 0;
  return set == 0 || set == (int)p.size();
}

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
template <bool MOMENTS>
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
  if constexpr (MOMENTS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out.s1[o * 3 + k] = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) out.s2[o * 6 + k] = 0;
  }
}

template <bool MOMENTS>
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
  // the moments of the point, from the q of its row (an invalid lane holds q = 0): m, then xx, xy, xz, yy, yz, zz
  long long v[MOMENTS ? 9 : 1];
  if constexpr (MOMENTS) {
    const long long m0 = q.x >> VM_MOMENT_SHIFT, m1 = q.y >> VM_MOMENT_SHIFT, m2 = q.z >> VM_MOMENT_SHIFT;
    v[0] = m0, v[1] = m1, v[2] = m2;
    v[3] = m0 * m0, v[4] = m0 * m1, v[5] = m0 * m2, v[6] = m1 * m1, v[7] = m1 * m2, v[8] = m2 * m2;
  }
  const WaveRun run = wave_run(bal);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long ax = __shfl_up(sx, d), ay = __shfl_up(sy, d), az = __shfl_up(sz, d);
    const int ac = __shfl_up(cnt, d), ao = __shfl_up(ob, d);
    long long av[MOMENTS ? 9 : 1];
    if constexpr (MOMENTS) {
#pragma unroll
      for (int k = 0; k < 9; ++k) av[k] = __shfl_up(v[k], d);
    }
    if (lane - d >= run.start) {
      sx += ax, sy += ay, sz += az, cnt += ac, ob += ao;
      if constexpr (MOMENTS) {
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] += av[k];
      }
    }
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
    if constexpr (MOMENTS) {
#pragma unroll
      for (int k = 0; k < 3; ++k) out.s1[o * 3 + k] = v[k];
#pragma unroll
      for (int k = 0; k < 6; ++k) out.s2[o * 6 + k] = v[3 + k];
    }
  } else {
    unsigned long long* dst = (unsigned long long*)(out.sums + o * 3);
    atomicAdd(dst, (unsigned long long)sx);
    atomicAdd(dst + 1, (unsigned long long)sy);
    atomicAdd(dst + 2, (unsigned long long)sz);
    atomicAdd(out.count + o, cnt);
    atomicAdd(out.obs + o, ob);
    if constexpr (MOMENTS) {
#pragma unroll
      for (int k = 0; k < 3; ++k) atomicAdd((unsigned long long*)(out.s1 + o * 3 + k), (unsigned long long)v[k]);
#pragma unroll
      for (int k = 0; k < 6; ++k) atomicAdd((unsigned long long*)(out.s2 + o * 6 + k), (unsigned long long)v[3 + k]);
    }
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

// row `from` of R to row `to` of out, moments included
template <bool MOMENTS>
__device__ static inline void vm_copy_row(const VmCRec& R, int64_t from, const VmRec& out, int64_t to) {
  out.keys[to] = R.keys[from];
  out.sums[to * 3] = R.sums[from * 3], out.sums[to * 3 + 1] = R.sums[from * 3 + 1], out.sums[to * 3 + 2] = R.sums[from * 3 + 2];
  out.count[to] = R.count[from];
  out.obs[to] = R.obs[from];
  if constexpr (MOMENTS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out.s1[to * 3 + k] = R.s1[from * 3 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) out.s2[to * 6 + k] = R.s2[from * 6 + k];
  }
}

template <bool MOMENTS>
__global__ __launch_bounds__(VM_WG) void mg_place_a_kernel(VmCRec A, const int64_t* __restrict__ n_a, int64_t cap_a,
                                                           const uint64_t* __restrict__ b_keys, const int64_t* __restrict__ n_b,
                                                           int64_t cap_b, const int32_t* __restrict__ rank, const int32_t* __restrict__ meta,
                                                           VmRec out, int64_t capacity_out) {
  const int64_t i = (int64_t)blockIdx.x * VM_WG + threadIdx.x;
  if (i >= vm_live(n_a, cap_a)) return;
  const uint64_t k = A.keys[i];
  const int64_t pos = meta[0] ? i + rank[vm_lower_bound(b_keys, vm_live(n_b, cap_b), k)] : i;      // the union does not fit: out = A
  if (pos >= capacity_out) return;            // cannot happen (mg_scan compared the total); keeps the stores in bounds regardless
  vm_copy_row<MOMENTS>(A, i, out, pos);
}

// after mg_place_a: a matched row adds into its partner's record (keys are unique: one B row per record, no atomic)
template <bool MOMENTS>
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
    if constexpr (MOMENTS) {
#pragma unroll
      for (int k = 0; k < 3; ++k) out.s1[pos * 3 + k] += B.s1[j * 3 + k];
#pragma unroll
      for (int k = 0; k < 6; ++k) out.s2[pos * 6 + k] += B.s2[j * 6 + k];
    }
  } else {
    vm_copy_row<MOMENTS>(B, j, out, pos);
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

// ------------------------------------------------------------------ subtract
static constexpr uint32_t SB_MATCHED = 0x80000000u;

// r = A[i] - B[j], field by field (the 64-bit sums wrap like the additions that made them)
struct SbRow {
  int64_t sums[3], s1[3], s2[6];
  int64_t count, obs;
};
template <bool MOMENTS>
__device__ static inline SbRow sb_diff(const VmCRec& A, int64_t i, const VmCRec& B, int64_t j) {
  SbRow r;
#pragma unroll
  for (int k = 0; k < 3; ++k) r.sums[k] = (int64_t)((uint64_t)A.sums[i * 3 + k] - (uint64_t)B.sums[j * 3 + k]);
  r.count = (int64_t)A.count[i] - (int64_t)B.count[j];
  r.obs = (int64_t)A.obs[i] - (int64_t)B.obs[j];
  if constexpr (MOMENTS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) r.s1[k] = (int64_t)((uint64_t)A.s1[i * 3 + k] - (uint64_t)B.s1[j * 3 + k]);
#pragma unroll
    for (int k = 0; k < 6; ++k) r.s2[k] = (int64_t)((uint64_t)A.s2[i * 6 + k] - (uint64_t)B.s2[j * 6 + k]);
  }
  return r;
}
template <bool MOMENTS>
__device__ static inline bool sb_all_zero(const SbRow& r) {
  int64_t any = r.sums[0] | r.sums[1] | r.sums[2] | r.count | r.obs;
  if constexpr (MOMENTS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) any |= r.s1[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) any |= r.s2[k];
  }
  return any == 0;
}

// every A row searches B: lb_b[i] = its partner's row | SB_MATCHED.  Per workgroup: rows that stay (a matched row whose
// remainder has count 0 leaves), matched rows, illegal rows
template <bool MOMENTS>
__global__ __launch_bounds__(VM_WG) void sb_flag_kernel(VmCRec A, const int64_t* __restrict__ n_a, int64_t cap_a, VmCRec B,
                                                        const int64_t* __restrict__ n_b, int64_t cap_b, uint32_t* __restrict__ lb_b,
                                                        int32_t* __restrict__ keepcnt, int32_t* __restrict__ matchcnt,
                                                        int32_t* __restrict__ badcnt) {
  const int64_t i = (int64_t)blockIdx.x * VM_WG + threadIdx.x;
  const int64_t na = vm_live(n_a, cap_a), nb = vm_live(n_b, cap_b);
  bool keep = false, matched = false, bad = false;
  if (i < na) {
    const uint64_t k = A.keys[i];
    const int64_t lb = vm_lower_bound(B.keys, nb, k);
    matched = lb < nb && B.keys[lb] == k;
    lb_b[i] = (uint32_t)lb | (matched ? SB_MATCHED : 0u);
    keep = true;
    if (matched) {
      const SbRow r = sb_diff<MOMENTS>(A, i, B, lb);
      keep = r.count != 0;
      bad = !(sb_all_zero<MOMENTS>(r) || (r.count > 0 && r.obs > 0));
    }
  }
  const int keeps = wg_count<VM_WG>(keep), matches = wg_count<VM_WG>(matched), bads = wg_count<VM_WG>(bad);
  if (threadIdx.x == 0) keepcnt[blockIdx.x] = keeps, matchcnt[blockIdx.x] = matches, badcnt[blockIdx.x] = bads;
}

// one workgroup: the scan of the staying rows, the verdict.  Fewer matched rows than B has rows: a B key is absent from A.
// meta[0] = 1: every B row is legal
__global__ __launch_bounds__(VM_WG) void sb_scan_kernel(int32_t* __restrict__ keepcnt, const int32_t* __restrict__ matchcnt,
                                                        const int32_t* __restrict__ badcnt, int64_t nblk,
                                                        const int64_t* __restrict__ n_a, int64_t cap_a, const int64_t* __restrict__ n_b,
                                                        int64_t cap_b, int64_t* __restrict__ n_out, int32_t* __restrict__ status,
                                                        int32_t* __restrict__ meta) {
  const int64_t kept = wg_scan<VM_WG>(keepcnt, nblk);
  __syncthreads();
  const int64_t matched = wg_scan<VM_WG>(nblk, [&](int64_t b) { return (int64_t)matchcnt[b]; }, [](int64_t, int64_t, int64_t) {});
  __syncthreads();
  const int64_t bad = wg_scan<VM_WG>(nblk, [&](int64_t b) { return (int64_t)badcnt[b]; }, [](int64_t, int64_t, int64_t) {});
  if (threadIdx.x == 0) {
    const bool fail = bad != 0 || matched != vm_live(n_b, cap_b);
    if (fail) atomicOr(status, EGONN_VMAP_STATUS_MISMATCH);
    *n_out = fail ? vm_live(n_a, cap_a) : kept;
    meta[0] = fail ? 0 : 1;
  }
}

// MISMATCH: out = A, row for row
template <bool MOMENTS>
__global__ __launch_bounds__(VM_WG) void sb_write_kernel(VmCRec A, const int64_t* __restrict__ n_a, int64_t cap_a, VmCRec B,
                                                         const uint32_t* __restrict__ lb_b, const int32_t* __restrict__ keeppre,
                                                         const int32_t* __restrict__ meta, VmRec out, int64_t capacity_out) {
  const int64_t i = (int64_t)blockIdx.x * VM_WG + threadIdx.x;
  const bool live = i < vm_live(n_a, cap_a), go = meta[0] != 0;
  const uint32_t e = live ? lb_b[i] : 0u;
  const bool matched = live && go && (e & SB_MATCHED);
  SbRow r;
  if (matched) r = sb_diff<MOMENTS>(A, i, B, (int64_t)(e & ~SB_MATCHED));
  const bool keep = live && !(matched && r.count == 0);
  const int64_t pos = go ? (int64_t)keeppre[blockIdx.x] + wg_rank<VM_WG>(__ballot(keep)) : i;        // go is uniform
  if (!keep || pos >= capacity_out) return;   // pos <= i < capacity_a <= capacity_out; keeps the stores in bounds regardless
  if (!matched) {
    vm_copy_row<MOMENTS>(A, i, out, pos);
    return;
  }
  out.keys[pos] = A.keys[i];
#pragma unroll
  for (int k = 0; k < 3; ++k) out.sums[pos * 3 + k] = r.sums[k];
  out.count[pos] = (int32_t)r.count;
  out.obs[pos] = (int32_t)r.obs;
  if constexpr (MOMENTS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out.s1[pos * 3 + k] = r.s1[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) out.s2[pos * 6 + k] = r.s2[k];
  }
}

struct SbSpan {
  int64_t nblk;             // workgroups over the A rows
  uint32_t* lb_b;
  int32_t *keepcnt, *matchcnt, *badcnt, *meta;
  size_t total;
};
static SbSpan sb_span(void* scratch, int64_t capacity_a) {
  SbSpan S;
  Carve c(scratch);
  const size_t m = (size_t)(capacity_a > 0 ? capacity_a : 1);
  S.nblk = cdiv((int64_t)m, VM_WG);
  S.lb_b = c.take<uint32_t>(m);
  S.keepcnt = c.take<int32_t>((size_t)S.nblk + 1);
  S.matchcnt = c.take<int32_t>((size_t)S.nblk);
  S.badcnt = c.take<int32_t>((size_t)S.nblk);
  S.meta = c.take<int32_t>(64);
  S.total = c.total();
  return S;
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

// integrate and integrate_moments: `who` names the entry point in its refusals
static int vm_integrate(const char* who, const double* bank, int64_t n_bank, const int64_t* bank_offsets, int64_t n_clouds,
                        const int32_t* pick, const double* poses, int n_obs, const double* origin, double voxel,
                        int64_t points_capacity, const VmRec& out, int64_t capacity, int64_t* n_out, int32_t* status, void* scratch,
                        int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(n_bank >= 0 && n_clouds >= 0 && n_clouds < (1ll << 31) && vm_integrate_shape_ok(points_capacity, n_obs) &&
                    capacity >= 0 && capacity < (1ll << 31),
                EGONN_ERR_INVALID, "%s: bad shape (n_bank=%lld, n_clouds=%lld, n_obs=%d in [1, %d], "
                "points_capacity=%lld, capacity=%lld; both < 2^31)", who, (long long)n_bank, (long long)n_clouds, n_obs, VM_MAX_OBS,
                (long long)points_capacity, (long long)capacity);
  EGONN_REQUIRE(vm_frame_ok(origin, voxel), EGONN_ERR_INVALID, "%s: voxel must be finite and > 0, origin finite", who);
  bool moments;
  EGONN_REQUIRE(vm_moments_agree({out.s1, out.s2}, &moments), EGONN_ERR_INVALID,
                "%s: the moment arrays s1 / s2 are all given or all null", who);
  EGONN_REQUIRE(bank_offsets && pick && poses && n_out && status && scratch && (n_bank == 0 || bank) &&
                    (capacity == 0 || (out.keys && out.sums && out.count && out.obs)),
                EGONN_ERR_INVALID, "%s: null pointer", who);
  VmSpan S = vm_span(scratch, points_capacity, n_obs);
  EGONN_TRY(span_check(who, scratch, scratch_bytes, S.total));
  hipStream_t st = (hipStream_t)stream;
  VmFrame F = {{origin[0], origin[1], origin[2]}, voxel};
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
  if (moments) {
    hipLaunchKernelGGL(vm_head_kernel<true>, grid, wg, 0, st, keys, total, points_capacity, S.blockcnt, S.meta, out, capacity);
    hipLaunchKernelGGL(vm_reduce_kernel<true>, grid, wg, 0, st, keys, vals, S.q4, total, points_capacity, S.blockcnt, S.meta, out,
                       capacity);
  } else {
    hipLaunchKernelGGL(vm_head_kernel<false>, grid, wg, 0, st, keys, total, points_capacity, S.blockcnt, S.meta, out, capacity);
    hipLaunchKernelGGL(vm_reduce_kernel<false>, grid, wg, 0, st, keys, vals, S.q4, total, points_capacity, S.blockcnt, S.meta, out,
                       capacity);
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_voxel_map_integrate(const double* bank, int64_t n_bank, const int64_t* bank_offsets, int64_t n_clouds, const int32_t* pick,
                                  const double* poses, int n_obs, const double* origin, double voxel, int64_t points_capacity,
                                  uint64_t* out_keys, int64_t* out_sums, int32_t* out_count, int32_t* out_obs, int64_t capacity,
                                  int64_t* n_out, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream) {
  return vm_integrate("voxel_map_integrate", bank, n_bank, bank_offsets, n_clouds, pick, poses, n_obs, origin, voxel, points_capacity,
                      {out_keys, out_sums, out_count, out_obs, nullptr, nullptr}, capacity, n_out, status, scratch, scratch_bytes,
                      stream);
}

API int64_t egonn_voxel_map_integrate_moments_scratch_bytes(int64_t points_capacity, int n_obs) {
  return egonn_voxel_map_integrate_scratch_bytes(points_capacity, n_obs);           // no extra per-point storage
}

API int egonn_voxel_map_integrate_moments(const double* bank, int64_t n_bank, const int64_t* bank_offsets, int64_t n_clouds,
                                          const int32_t* pick, const double* poses, int n_obs, const double* origin, double voxel,
                                          int64_t points_capacity, uint64_t* out_keys, int64_t* out_sums, int32_t* out_count,
                                          int32_t* out_obs, int64_t* out_s1, int64_t* out_s2, int64_t capacity, int64_t* n_out,
                                          int32_t* status, void* scratch, int64_t scratch_bytes, void* stream) {
  return vm_integrate("voxel_map_integrate_moments", bank, n_bank, bank_offsets, n_clouds, pick, poses, n_obs, origin, voxel,
                      points_capacity, {out_keys, out_sums, out_count, out_obs, out_s1, out_s2}, capacity, n_out, status, scratch,
                      scratch_bytes, stream);
}

API int64_t egonn_voxel_map_merge_scratch_bytes(int64_t capacity_a, int64_t capacity_b, int64_t capacity_out) {
  if (!mg_shape_ok(capacity_a, capacity_b, capacity_out)) return -1;
  return (int64_t)mg_span(nullptr, capacity_b).total;
}

// what merge, merge_moments and subtract ask of their three record sets
static int vm_binary_check(const char* who, const VmCRec& A, const int64_t* n_a, int64_t capacity_a, const VmCRec& B, const int64_t* n_b,
                           int64_t capacity_b, const VmRec& out, int64_t capacity_out, const int64_t* n_out, const int32_t* status,
                           const void* scratch, bool* moments) {
  EGONN_REQUIRE(mg_shape_ok(capacity_a, capacity_b, capacity_out), EGONN_ERR_INVALID,
                "%s: bad shape (capacity_a=%lld, capacity_b=%lld, capacity_out=%lld >= capacity_a; all < 2^31)", who,
                (long long)capacity_a, (long long)capacity_b, (long long)capacity_out);
  EGONN_REQUIRE(vm_moments_agree({A.s1, A.s2, B.s1, B.s2, out.s1, out.s2}, moments), EGONN_ERR_INVALID,
                "%s: the moment arrays s1 / s2 of A, B and out are all given or all null", who);
  EGONN_REQUIRE(n_a && n_b && n_out && status && scratch && (capacity_a == 0 || (A.keys && A.sums && A.count && A.obs)) &&
                    (capacity_b == 0 || (B.keys && B.sums && B.count && B.obs)) &&
                    (capacity_out == 0 || (out.keys && out.sums && out.count && out.obs)),
                EGONN_ERR_INVALID, "%s: null pointer", who);
  EGONN_REQUIRE(capacity_out == 0 || (out.keys != A.keys && out.keys != B.keys), EGONN_ERR_INVALID, "%s: out must not be A or B", who);
  return EGONN_OK;
}

static int vm_merge(const char* who, const VmCRec& A, const int64_t* n_a, int64_t capacity_a, const VmCRec& B, const int64_t* n_b,
                    int64_t capacity_b, const VmRec& out, int64_t capacity_out, int64_t* n_out, int32_t* status, void* scratch,
                    int64_t scratch_bytes, void* stream) {
  bool moments;
  EGONN_TRY(vm_binary_check(who, A, n_a, capacity_a, B, n_b, capacity_b, out, capacity_out, n_out, status, scratch, &moments));
  const MgSpan S = mg_span(scratch, capacity_b);
  EGONN_TRY(span_check(who, scratch, scratch_bytes, S.total));
  hipStream_t st = (hipStream_t)stream;
  const dim3 wg(VM_WG), grid_a((unsigned)cdiv(capacity_a, VM_WG)), grid_b((unsigned)S.nblk);
  hipLaunchKernelGGL(mg_search_kernel, grid_b, wg, 0, st, A.keys, n_a, capacity_a, B.keys, n_b, capacity_b, S.lb_a, S.blockcnt);
  hipLaunchKernelGGL(mg_scan_kernel, dim3(1), wg, 0, st, S.blockcnt, S.nblk, n_a, capacity_a, capacity_out, n_out, status, S.meta);
  hipLaunchKernelGGL(mg_rank_kernel, dim3((unsigned)cdiv(capacity_b + 1, VM_WG)), wg, 0, st, S.lb_a, n_b, capacity_b, S.blockcnt, S.meta,
                     S.rank);
  if (capacity_a > 0) {
    if (moments)
      hipLaunchKernelGGL(mg_place_a_kernel<true>, grid_a, wg, 0, st, A, n_a, capacity_a, B.keys, n_b, capacity_b, S.rank, S.meta, out,
                         capacity_out);
    else
      hipLaunchKernelGGL(mg_place_a_kernel<false>, grid_a, wg, 0, st, A, n_a, capacity_a, B.keys, n_b, capacity_b, S.rank, S.meta, out,
                         capacity_out);
  }
  if (capacity_b > 0) {
    if (moments)
      hipLaunchKernelGGL(mg_place_b_kernel<true>, grid_b, wg, 0, st, B, n_b, capacity_b, S.lb_a, S.rank, S.meta, out, capacity_out);
    else
      hipLaunchKernelGGL(mg_place_b_kernel<false>, grid_b, wg, 0, st, B, n_b, capacity_b, S.lb_a, S.rank, S.meta, out, capacity_out);
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_voxel_map_merge(const uint64_t* a_keys, const int64_t* a_sums, const int32_t* a_count, const int32_t* a_obs,
                              const int64_t* n_a, int64_t capacity_a, const uint64_t* b_keys, const int64_t* b_sums,
                              const int32_t* b_count, const int32_t* b_obs, const int64_t* n_b, int64_t capacity_b, uint64_t* out_keys,
                              int64_t* out_sums, int32_t* out_count, int32_t* out_obs, int64_t capacity_out, int64_t* n_out,
                              int32_t* status, void* scratch, int64_t scratch_bytes, void* stream) {
  return vm_merge("voxel_map_merge", {a_keys, a_sums, a_count, a_obs, nullptr, nullptr}, n_a, capacity_a,
                  {b_keys, b_sums, b_count, b_obs, nullptr, nullptr}, n_b, capacity_b,
                  {out_keys, out_sums, out_count, out_obs, nullptr, nullptr}, capacity_out, n_out, status, scratch, scratch_bytes, stream);
}

API int64_t egonn_voxel_map_merge_moments_scratch_bytes(int64_t capacity_a, int64_t capacity_b, int64_t capacity_out) {
  return egonn_voxel_map_merge_scratch_bytes(capacity_a, capacity_b, capacity_out);
}

API int egonn_voxel_map_merge_moments(const uint64_t* a_keys, const int64_t* a_sums, const int32_t* a_count, const int32_t* a_obs,
                                      const int64_t* a_s1, const int64_t* a_s2, const int64_t* n_a, int64_t capacity_a,
                                      const uint64_t* b_keys, const int64_t* b_sums, const int32_t* b_count, const int32_t* b_obs,
                                      const int64_t* b_s1, const int64_t* b_s2, const int64_t* n_b, int64_t capacity_b,
                                      uint64_t* out_keys, int64_t* out_sums, int32_t* out_count, int32_t* out_obs, int64_t* out_s1,
                                      int64_t* out_s2, int64_t capacity_out, int64_t* n_out, int32_t* status, void* scratch,
                                      int64_t scratch_bytes, void* stream) {
  return vm_merge("voxel_map_merge_moments", {a_keys, a_sums, a_count, a_obs, a_s1, a_s2}, n_a, capacity_a,
                  {b_keys, b_sums, b_count, b_obs, b_s1, b_s2}, n_b, capacity_b, {out_keys, out_sums, out_count, out_obs, out_s1, out_s2},
                  capacity_out, n_out, status, scratch, scratch_bytes, stream);
}

API int64_t egonn_voxel_map_subtract_scratch_bytes(int64_t capacity_a, int64_t capacity_b, int64_t capacity_out) {
  if (!mg_shape_ok(capacity_a, capacity_b, capacity_out)) return -1;
  return (int64_t)sb_span(nullptr, capacity_a).total;
}

API int egonn_voxel_map_subtract(const uint64_t* a_keys, const int64_t* a_sums, const int32_t* a_count, const int32_t* a_obs,
                                 const int64_t* a_s1, const int64_t* a_s2, const int64_t* n_a, int64_t capacity_a,
                                 const uint64_t* b_keys, const int64_t* b_sums, const int32_t* b_count, const int32_t* b_obs,
                                 const int64_t* b_s1, const int64_t* b_s2, const int64_t* n_b, int64_t capacity_b, uint64_t* out_keys,
                                 int64_t* out_sums, int32_t* out_count, int32_t* out_obs, int64_t* out_s1, int64_t* out_s2,
                                 int64_t capacity_out, int64_t* n_out, int32_t* status, void* scratch, int64_t scratch_bytes,
                                 void* stream) {
  const char* who = "voxel_map_subtract";
  const VmCRec A = {a_keys, a_sums, a_count, a_obs, a_s1, a_s2}, B = {b_keys, b_sums, b_count, b_obs, b_s1, b_s2};
  const VmRec out = {out_keys, out_sums, out_count, out_obs, out_s1, out_s2};
  bool moments;
  EGONN_TRY(vm_binary_check(who, A, n_a, capacity_a, B, n_b, capacity_b, out, capacity_out, n_out, status, scratch, &moments));
  const SbSpan S = sb_span(scratch, capacity_a);
  EGONN_TRY(span_check(who, scratch, scratch_bytes, S.total));
  hipStream_t st = (hipStream_t)stream;
  const dim3 wg(VM_WG), grid((unsigned)S.nblk);
  if (moments)
    hipLaunchKernelGGL(sb_flag_kernel<true>, grid, wg, 0, st, A, n_a, capacity_a, B, n_b, capacity_b, S.lb_b, S.keepcnt, S.matchcnt,
                       S.badcnt);
  else
    hipLaunchKernelGGL(sb_flag_kernel<false>, grid, wg, 0, st, A, n_a, capacity_a, B, n_b, capacity_b, S.lb_b, S.keepcnt, S.matchcnt,
                       S.badcnt);
  hipLaunchKernelGGL(sb_scan_kernel, dim3(1), wg, 0, st, S.keepcnt, S.matchcnt, S.badcnt, S.nblk, n_a, capacity_a, n_b, capacity_b, n_out,
                     status, S.meta);
  if (moments)
    hipLaunchKernelGGL(sb_write_kernel<true>, grid, wg, 0, st, A, n_a, capacity_a, B, S.lb_b, S.keepcnt, S.meta, out, capacity_out);
  else
    hipLaunchKernelGGL(sb_write_kernel<false>, grid, wg, 0, st, A, n_a, capacity_a, B, S.lb_b, S.keepcnt, S.meta, out, capacity_out);
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
