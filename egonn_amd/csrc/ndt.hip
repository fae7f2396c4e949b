// The NDT layer on the voxel map: second moments per voxel (accumulate), one Gaussian per voxel (finalize), scan-to-map
// registration against the Gaussians (register).  DESIGN.md §3.20; the arithmetic is stated once in include/egonn_hip.h ("NDT
// layer") and restated in numpy in tests/ndt_ref.py.
//
// The layer lies over a fixed, ascending key array (a snapshot of a voxel map's keys).  A point's key and residuals are the
// voxel map's, bit for bit (voxel_key.h); its moments are integers, so accumulating in any number of calls and in any order
// gives the bits of one call.  There is no floating-point atomic in this file.
//
// accumulate  vm_offsets (voxel_key.h), ndt_accumulate: key, binary search, equal consecutive rows combined inside a wave by a
//             segmented scan (the bank's clouds are in voxel order: consecutive lanes often share a row; the run bounds are
//             compact.h's wave_run); the last lane of a run issues ten integer atomics.
// finalize    one lane per row: mean, covariance, cyclic Jacobi (jacobi3.h), the eigenvalue floor, the information matrix.
// register    ndt_setup (pairs, the workgroup table), then max_iteration + 1 rounds of ndt_eval (256 consecutive source points
//             of one pair per workgroup: up to seven lookups per point, 30 partial sums in a fixed tree) and ndt_finish (one
//             workgroup per pair: partials in ascending order, the stop rule, the 6 x 6 step of plane_step.h).  A stopped
//             pair's workgroups return at once.  No call synchronises with the host.  The loop itself (per-pair state, the flat
//             grid, the tree, the gather, stop and advance) is pair_loop.h, shared with icp.hip; this file supplies the terms
//             of a point, the stop rule on the step's size and the step.
#include "../../include/egonn_hip.h"
#include "common.h"
#include "compact.h"
#include "jacobi3.h"
#include "pair_loop.h"
#include "plane_step.h"
#include "voxel_key.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int NDT_WG = PAIR_WG;
static constexpr int NDT_NPART = 30;             // n_term, n_pts, A (21 upper entries row by row), b (6), score: the layout of
                                                 // icp_plane_solve at [2, 29)
static constexpr int NDT_MOMENT_SHIFT = 10;      // m = q >> 10: 20 bits, so 2^23 squares fit an int64

// ------------------------------------------------------------------ accumulate
__global__ __launch_bounds__(NDT_WG) void ndt_accumulate_kernel(const double* __restrict__ bank, int64_t n_bank,
                                                                const int64_t* __restrict__ off, int64_t n_clouds,
                                                                const int32_t* __restrict__ pick, const double* __restrict__ poses,
                                                                int n_obs, VmFrame F, const int64_t* __restrict__ obs_off, int64_t cap,
                                                                const uint64_t* __restrict__ keys, const int64_t* __restrict__ n_dev,
                                                                int64_t capacity_map, int32_t* __restrict__ cnt,
                                                                int64_t* __restrict__ s1, int64_t* __restrict__ s2,
                                                                int64_t* __restrict__ missed, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * NDT_WG + threadIdx.x;
  const int64_t total = clipi(obs_off[n_obs], cap), n = vm_live(n_dev, capacity_map);
  int64_t row = -1;
  bool miss = false, bad = false;
  long long v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (i < total) {
    int64_t src;
    const int k = vm_point_source(obs_off, n_obs, off, n_bank, n_clouds, pick, i, &src);
    uint64_t key = VM_INVALID;
    int r[3];
    if (src >= 0 && vm_point_key(bank + src * 3, poses + (int64_t)k * 16, F, &key, r)) {
      const int64_t lb = vm_lower_bound(keys, n, key);
      if (lb < n && keys[lb] == key) {
        row = lb;
        const long long m0 = r[0] >> NDT_MOMENT_SHIFT, m1 = r[1] >> NDT_MOMENT_SHIFT, m2 = r[2] >> NDT_MOMENT_SHIFT;
        v[0] = m0, v[1] = m1, v[2] = m2;
        v[3] = m0 * m0, v[4] = m0 * m1, v[5] = m0 * m2, v[6] = m1 * m1, v[7] = m1 * m2, v[8] = m2 * m2;
      } else {
        miss = true;
      }
    } else {
      bad = true;
    }
  }
  if (bad) atomicOr(status, EGONN_VMAP_STATUS_RANGE);
  const unsigned long long mbal = __ballot(miss);
  if (lane == 0 && mbal) atomicAdd((unsigned long long*)missed, (unsigned long long)__popcll(mbal));
  // runs of equal rows in consecutive lanes: a segmented scan bounded by the run's first lane
  const long long prev = __shfl_up((long long)row, 1), next = __shfl_down((long long)row, 1);
  const bool head = row >= 0 && (lane == 0 || prev != row);
  const unsigned long long bal = __ballot(head);
  if (__ballot(row >= 0) == 0ull) return;                                   // wave-uniform
  const WaveRun run = wave_run(bal);
  int c = row >= 0 ? 1 : 0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int ac = __shfl_up(c, d);
    long long a[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) a[k] = __shfl_up(v[k], d);
    if (lane - d >= run.start) {
      c += ac;
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] += a[k];
    }
  }
  if (row < 0 || row >= capacity_map || (lane < 63 && next == row)) return;  // the last lane of a run holds the run's sums
  atomicAdd(cnt + row, c);
#pragma unroll
  for (int k = 0; k < 3; ++k) atomicAdd((unsigned long long*)(s1 + row * 3 + k), (unsigned long long)v[k]);
#pragma unroll
  for (int k = 0; k < 6; ++k) atomicAdd((unsigned long long*)(s2 + row * 6 + k), (unsigned long long)v[3 + k]);
}

// ------------------------------------------------------------------ finalize
__global__ __launch_bounds__(NDT_WG) void ndt_finalize_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ n_dev,
                                                              int64_t capacity_map, const int32_t* __restrict__ cnt,
                                                              const int64_t* __restrict__ s1, const int64_t* __restrict__ s2,
                                                              double voxel, int min_points, double min_eig_ratio,
                                                              double* __restrict__ mean, double* __restrict__ info,
                                                              double* __restrict__ eigenvalues, double* __restrict__ normal,
                                                              uint8_t* __restrict__ valid, int64_t* __restrict__ n_valid,
                                                              double* __restrict__ cov) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * NDT_WG + threadIdx.x;
  const bool live = i < vm_live(n_dev, capacity_map);
  bool good = false;
  if (live) {
    const uint64_t key = keys[i];
    const int32_t ci = cnt[i];
    const double nf = (double)ci, u = voxel * 0x1p-20;
    double a1[3], mu[3], C[6], A[3][3], V[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int64_t idx = (int64_t)((key >> ((2 - a) * VM_BITS)) & VM_MASK) - VM_BIAS;
      a1[a] = (double)s1[i * 3 + a];
      mu[a] = ((double)idx + (a1[a] / nf) * 0x1p-20) * voxel;
    }
    {
      int e = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b, ++e) {
          C[e] = ((((double)s2[i * 6 + e] - (a1[a] * a1[b]) / nf) / (nf - 1.0)) * u) * u;
          A[a][b] = A[b][a] = C[e];
        }
    }
    nrm_jacobi3(A, V);
    const double l[3] = {A[0][0], A[1][1], A[2][2]};
    int p0 = 0, p1 = 1, p2 = 2, sw;                      // ascending, ties in column order: a stable bubble sort
    if (l[p1] < l[p0]) sw = p0, p0 = p1, p1 = sw;
    if (l[p2] < l[p1]) sw = p1, p1 = p2, p2 = sw;
    if (l[p1] < l[p0]) sw = p0, p0 = p1, p1 = sw;
    const int ord[3] = {p0, p1, p2};
    double ev[3], vec[3][3];                             // vec[i] = eigenvector i
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int o = ord[k];
      ev[k] = o == 0 ? l[0] : (o == 1 ? l[1] : l[2]);
#pragma unroll
      for (int a = 0; a < 3; ++a) vec[k][a] = o == 0 ? V[a][0] : (o == 1 ? V[a][1] : V[a][2]);
    }
    const double floor_l = min_eig_ratio * ev[2];
    double I6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double w = 1.0 / (ev[k] > floor_l ? ev[k] : floor_l);       // l' = max(l, min_eig_ratio * l_2)
      int e = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b, ++e) I6[e] += (w * vec[k][a]) * vec[k][b];
    }
    double nx = vec[0][0], ny = vec[0][1], nz = vec[0][2];
    const double lead = nx != 0.0 ? nx : (ny != 0.0 ? ny : nz);
    if (lead < 0.0) nx = -nx, ny = -ny, nz = -nz;
    good = ci >= min_points && ev[2] > 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) good = good && fabs(mu[k]) < INFINITY && fabs(ev[k]) < INFINITY;       // false for NaN
#pragma unroll
    for (int k = 0; k < 6; ++k) good = good && fabs(C[k]) < INFINITY && fabs(I6[k]) < INFINITY;
    good = good && fabs(nx) < INFINITY && fabs(ny) < INFINITY && fabs(nz) < INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      mean[i * 3 + k] = good ? mu[k] : 0.0;
      eigenvalues[i * 3 + k] = good ? ev[k] : 0.0;
    }
    normal[i * 3] = good ? nx : 0.0, normal[i * 3 + 1] = good ? ny : 0.0, normal[i * 3 + 2] = good ? nz : 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      info[i * 6 + k] = good ? I6[k] : 0.0;
      if (cov) cov[i * 6 + k] = good ? C[k] : 0.0;
    }
    valid[i] = good ? 1 : 0;
  }
  const unsigned long long bal = __ballot(good);
  if (lane == 0 && bal) atomicAdd((unsigned long long*)n_valid, (unsigned long long)__popcll(bal));
}

// ------------------------------------------------------------------ register
struct NdtPair {            // the members pair_loop.h asks for, and conv
  double R[9], t[3];        // T_k
  int64_t so;               // first source point
  int32_t ns, done, status, conv;      // conv: the last step was below both epsilons
};

struct NdtLayer {
  const uint64_t* keys;
  const int64_t* n_dev;
  int64_t capacity_map;
  const double* mean;       // (rows, 3)
  const double* info;       // (rows, 6)
  const uint8_t* valid;
};

__global__ __launch_bounds__(NDT_WG) void ndt_setup_kernel(const int64_t* __restrict__ soff, int64_t ns_cap, int P,
                                                           const double* __restrict__ T_init, NdtPair* __restrict__ pairs,
                                                           int32_t* __restrict__ wg0, double* __restrict__ T_out,
                                                           double* __restrict__ fitness, double* __restrict__ score,
                                                           int32_t* __restrict__ iterations, int32_t* __restrict__ status,
                                                           double* __restrict__ T_trace, int max_it) {
  const int p = blockIdx.x * NDT_WG + threadIdx.x;
  if (p >= P) return;
  NdtPair q;
  pair_begin(&q, soff, ns_cap, P, p, T_init, T_trace, max_it, wg0);
  q.conv = 0;
  if (q.ns == 0) {
    pair_stop(&q, p, 0, EGONN_ICP_STATUS_EMPTY, T_out, iterations, status);
    fitness[p] = 0.0, score[p] = 0.0;
  }
  pairs[p] = q;
}

// one term: the Gaussian of `row` seen from vs; adds into the lane's sums v
__device__ static __forceinline__ bool ndt_term(const NdtLayer& M, int64_t row, const double* vs, double* v) {
  if (!M.valid[row]) return false;
  const double* mu = M.mean + row * 3;
  const double* I = M.info + row * 6;
  const double r0 = vs[0] - mu[0], r1 = vs[1] - mu[1], r2 = vs[2] - mu[2];
  const double I00 = I[0], I01 = I[1], I02 = I[2], I11 = I[3], I12 = I[4], I22 = I[5];
  const double g0 = (I00 * r0 + I01 * r1) + I02 * r2, g1 = (I01 * r0 + I11 * r1) + I12 * r2, g2 = (I02 * r0 + I12 * r1) + I22 * r2;
  const double m = (r0 * g0 + r1 * g1) + r2 * g2;
  if (!(fabs(m) < INFINITY)) return false;               // false for NaN
  const double w = exp(-0.5 * m);
  // J = [-[vs]x | I]: its columns j_c = e_c x vs (c < 3) and e_c; H_c = info j_c
  const double x = vs[0], y = vs[1], z = vs[2];
  const double J[6][3] = {{0.0, -z, y}, {z, 0.0, -x}, {-y, x, 0.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  double H[6][3];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    H[c][0] = (I00 * J[c][0] + I01 * J[c][1]) + I02 * J[c][2];
    H[c][1] = (I01 * J[c][0] + I11 * J[c][1]) + I12 * J[c][2];
    H[c][2] = (I02 * J[c][0] + I12 * J[c][1]) + I22 * J[c][2];
  }
  int e = 2;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) v[e++] += w * ((J[a][0] * H[b][0] + J[a][1] * H[b][1]) + J[a][2] * H[b][2]);
#pragma unroll
  for (int a = 0; a < 6; ++a) v[23 + a] += w * ((J[a][0] * g0 + J[a][1] * g1) + J[a][2] * g2);
  v[29] += w;
  v[0] += 1.0;
  return true;
}

template <int NB>
__global__ __launch_bounds__(NDT_WG) void ndt_eval_kernel(const NdtPair* __restrict__ pairs, const int32_t* __restrict__ wg0, int P,
                                                          const double* __restrict__ src, NdtLayer M, double voxel,
                                                          double* __restrict__ partial) {
  __shared__ double s_red[NDT_NPART][4];
  const int flat = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int p = pair_of(wg0, P, flat);
  const NdtPair* q = pairs + p;
  const int chunk = pair_chunk(q, wg0[p], flat);
  if (chunk < 0) return;                                  // workgroup-uniform
  const int row = chunk * NDT_WG + t;
  double v[NDT_NPART];
#pragma unroll
  for (int k = 0; k < NDT_NPART; ++k) v[k] = 0.0;
  if (row < q->ns) {
    double vs[3], f[3];
    bool ok = true;
    pair_apply(q, src + (q->so + row) * 3, vs);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      f[a] = floor(vs[a] / voxel);
      ok = ok && f[a] >= -(double)VM_BIAS - 1.0 && f[a] <= (double)VM_BIAS;      // beyond: no neighbour is in range; false for NaN
    }
    if (ok) {
      const int64_t n = vm_live(M.n_dev, M.capacity_map);
      const int64_t ix = (int64_t)f[0], iy = (int64_t)f[1], iz = (int64_t)f[2];
      auto in = [](int64_t a) { return a >= -VM_BIAS && a < VM_BIAS; };
      auto key_of = [](int64_t a, int64_t b, int64_t c) {
        const uint64_t idx[3] = {(uint64_t)(a + VM_BIAS), (uint64_t)(b + VM_BIAS), (uint64_t)(c + VM_BIAS)};
        return vm_pack_key(idx);
      };
      auto find = [&](int64_t a, int64_t b, int64_t c) -> int64_t {
        if (!(in(a) && in(b) && in(c))) return -1;
        const uint64_t k = key_of(a, b, c);
        const int64_t lb = vm_lower_bound(M.keys, n, k);
        return lb < n && M.keys[lb] == k ? lb : -1;
      };
      bool any = false;
      // the centre; its z neighbours are the rows next to where its key sits (keys are x-major, z is the lowest field)
      int64_t lb = 0;
      const bool cin = in(ix) && in(iy) && in(iz);
      uint64_t kc = 0;
      bool chit = false;
      if (cin) {
        kc = key_of(ix, iy, iz);
        lb = vm_lower_bound(M.keys, n, kc);
        chit = lb < n && M.keys[lb] == kc;
        if (chit) any = ndt_term(M, lb, vs, v) || any;
      }
      if constexpr (NB == 7) {
        const int64_t r1 = find(ix + 1, iy, iz), r2 = find(ix - 1, iy, iz), r3 = find(ix, iy + 1, iz), r4 = find(ix, iy - 1, iz);
        if (r1 >= 0) any = ndt_term(M, r1, vs, v) || any;
        if (r2 >= 0) any = ndt_term(M, r2, vs, v) || any;
        if (r3 >= 0) any = ndt_term(M, r3, vs, v) || any;
        if (r4 >= 0) any = ndt_term(M, r4, vs, v) || any;
        int64_t r5, r6;
        if (cin) {
          const int64_t up = chit ? lb + 1 : lb, dn = lb - 1;
          r5 = in(iz + 1) && up < n && M.keys[up] == kc + 1 ? up : -1;
          r6 = in(iz - 1) && dn >= 0 && M.keys[dn] == kc - 1 ? dn : -1;
        } else {
          r5 = find(ix, iy, iz + 1), r6 = find(ix, iy, iz - 1);
        }
        if (r5 >= 0) any = ndt_term(M, r5, vs, v) || any;
        if (r6 >= 0) any = ndt_term(M, r6, vs, v) || any;
      }
      v[1] = any ? 1.0 : 0.0;
    }
  }
  pair_reduce<NDT_NPART>(v, s_red, partial, flat, lane, w);
}

__global__ __launch_bounds__(64) void ndt_finish_kernel(NdtPair* __restrict__ pairs, const int32_t* __restrict__ wg0,
                                                        const double* __restrict__ partial, int round, int max_it, double eps_rot,
                                                        double eps_trans, double* __restrict__ T_out, double* __restrict__ fitness,
                                                        double* __restrict__ score, int32_t* __restrict__ iterations,
                                                        int32_t* __restrict__ status, double* __restrict__ T_trace,
                                                        double* __restrict__ eval_trace, double* __restrict__ sums_trace) {
  __shared__ double s[NDT_NPART];
  const int p = blockIdx.x, t = threadIdx.x;
  NdtPair* q = pairs + p;
  if (q->done) return;
  pair_gather<NDT_NPART>(q, wg0[p], partial, s);
  if (t != 0) return;
  const double n_term = s[0], n_pts = s[1], sc = s[29];
  int stop = 0, st = q->status;
  double x[6];
  if (q->conv) stop = 1;
  else if (round >= max_it) stop = 1, st |= EGONN_ICP_STATUS_MAX_ITER;
  else if (n_term < 6.0) stop = 1, st |= EGONN_ICP_STATUS_FEW_CORR;
  else if (!icp_plane_solve(s, x)) stop = 1, st |= EGONN_ICP_STATUS_SINGULAR;
  if (eval_trace) {
    double* e = eval_trace + ((size_t)p * (max_it + 1) + round) * 4;
    e[0] = n_term, e[1] = n_pts, e[2] = sc, e[3] = (double)stop;
  }
  if (sums_trace)
    for (int k = 0; k < NDT_NPART; ++k) sums_trace[((size_t)p * (max_it + 1) + round) * NDT_NPART + k] = s[k];
  if (stop) {
    fitness[p] = n_pts / (double)q->ns, score[p] = sc / (double)q->ns;
    pair_stop(q, p, round, st, T_out, iterations, status);
    return;
  }
  double U[9], ut[3];
  icp_plane_update(x, U, ut);
  const double mr = fmax(fmax(fabs(x[0]), fabs(x[1])), fabs(x[2])), mt = fmax(fmax(fabs(x[3]), fabs(x[4])), fabs(x[5]));
  q->conv = mr < eps_rot && mt < eps_trans ? 1 : 0;
  pair_advance(q, p, round, max_it, U, ut, T_trace);
}

static bool ndt_register_shape_ok(int64_t n_src, int n_pairs) {
  return n_src >= 0 && n_src < (1ll << 31) && n_pairs >= 1 && n_pairs <= EGONN_MAX_BATCH;
}
static bool ndt_pos(double x) { return x > 0.0 && x < INFINITY; }          // false for NaN

// The carves of register's scratch (accumulate's is one array: obs_off).  With scratch = nullptr only `total` means anything
struct NdtSpan {
  int64_t n_wg;             // workgroups of the flat grid
  NdtPair* pairs;
  int32_t* wg0;
  double* partial;
  size_t total;
};
static NdtSpan ndt_register_span(void* scratch, int64_t n_src, int n_pairs) {
  NdtSpan S;
  Carve c(scratch);
  const PairLayout L = pair_layout(c, n_src, n_pairs, sizeof(NdtPair));
  S.n_wg = L.n_wg, S.pairs = (NdtPair*)L.pairs, S.wg0 = L.wg0;
  S.partial = c.take<double>((size_t)L.n_wg * NDT_NPART);
  S.total = c.total();
  return S;
}

}  // namespace egonn

using namespace egonn;

// ------------------------------------------------------------------ entry points
API int64_t egonn_ndt_accumulate_scratch_bytes(int64_t points_capacity, int n_obs) {
  if (!vm_integrate_shape_ok(points_capacity, n_obs)) return -1;
  Carve c;
  c.take<int64_t>((size_t)n_obs + 1);
  return (int64_t)c.total();
}

API int egonn_ndt_accumulate(const double* bank, int64_t n_bank, const int64_t* bank_offsets, int64_t n_clouds, const int32_t* pick,
                             const double* poses, int n_obs, const double* origin, double voxel, int64_t points_capacity,
                             const uint64_t* keys, const int64_t* n_dev, int64_t capacity_map, int32_t* cnt, int64_t* s1, int64_t* s2,
                             int64_t* missed, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(n_bank >= 0 && n_clouds >= 0 && n_clouds < (1ll << 31) && vm_integrate_shape_ok(points_capacity, n_obs) &&
                    capacity_map >= 0 && capacity_map < (1ll << 31),
                EGONN_ERR_INVALID, "ndt_accumulate: bad shape (n_bank=%lld, n_clouds=%lld, n_obs=%d in [1, %d], "
                "points_capacity=%lld, capacity_map=%lld; both < 2^31)", (long long)n_bank, (long long)n_clouds, n_obs, VM_MAX_OBS,
                (long long)points_capacity, (long long)capacity_map);
  EGONN_REQUIRE(vm_frame_ok(origin, voxel), EGONN_ERR_INVALID, "ndt_accumulate: voxel must be finite and > 0, origin finite");
  EGONN_REQUIRE(bank_offsets && pick && poses && n_dev && missed && status && scratch && (n_bank == 0 || bank) &&
                    (capacity_map == 0 || (keys && cnt && s1 && s2)),
                EGONN_ERR_INVALID, "ndt_accumulate: null pointer");
  Carve c(scratch);
  int64_t* obs_off = c.take<int64_t>((size_t)n_obs + 1);
  EGONN_TRY(span_check("ndt_accumulate", scratch, scratch_bytes, c.total()));
  hipStream_t st = (hipStream_t)stream;
  VmFrame F = {{origin[0], origin[1], origin[2]}, voxel};
  hipLaunchKernelGGL(vm_offsets_kernel, dim3(1), dim3(VM_WG), 0, st, bank_offsets, n_bank, n_clouds, pick, n_obs, points_capacity,
                     obs_off, status);
  if (points_capacity > 0)
    hipLaunchKernelGGL(ndt_accumulate_kernel, dim3((unsigned)cdiv(points_capacity, NDT_WG)), dim3(NDT_WG), 0, st, bank, n_bank,
                       bank_offsets, n_clouds, pick, poses, n_obs, F, obs_off, points_capacity, keys, n_dev, capacity_map, cnt, s1, s2,
                       missed, status);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_ndt_finalize(const uint64_t* keys, const int64_t* n_dev, int64_t capacity_map, const int32_t* cnt, const int64_t* s1,
                           const int64_t* s2, double voxel, int min_points, double min_eig_ratio, double* mean, double* info,
                           double* eigenvalues, double* normal, uint8_t* valid, int64_t* n_valid, double* cov, void* stream) {
  EGONN_REQUIRE(capacity_map >= 0 && capacity_map < (1ll << 31), EGONN_ERR_INVALID,
                "ndt_finalize: bad shape (capacity_map=%lld; < 2^31)", (long long)capacity_map);
  EGONN_REQUIRE(ndt_pos(voxel), EGONN_ERR_INVALID, "ndt_finalize: voxel must be finite and > 0");
  EGONN_REQUIRE(min_points >= 3, EGONN_ERR_INVALID, "ndt_finalize: min_points %d below 3", min_points);
  EGONN_REQUIRE(ndt_pos(min_eig_ratio), EGONN_ERR_INVALID, "ndt_finalize: min_eig_ratio must be finite and > 0");
  EGONN_REQUIRE(n_dev && n_valid && (capacity_map == 0 || (keys && cnt && s1 && s2 && mean && info && eigenvalues && normal && valid)),
                EGONN_ERR_INVALID, "ndt_finalize: null pointer");
  hipStream_t st = (hipStream_t)stream;
  HIP_CHECK(hipMemsetAsync(n_valid, 0, sizeof(int64_t), st));
  if (capacity_map > 0)
    hipLaunchKernelGGL(ndt_finalize_kernel, dim3((unsigned)cdiv(capacity_map, NDT_WG)), dim3(NDT_WG), 0, st, keys, n_dev, capacity_map,
                       cnt, s1, s2, voxel, min_points, min_eig_ratio, mean, info, eigenvalues, normal, valid, n_valid, cov);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int64_t egonn_ndt_register_scratch_bytes(int64_t n_src, int n_pairs) {
  if (!ndt_register_shape_ok(n_src, n_pairs)) return -1;
  return (int64_t)ndt_register_span(nullptr, n_src, n_pairs).total;
}

API int egonn_ndt_register(const double* src, int64_t n_src, const int64_t* src_offsets, int n_pairs, const double* T_init,
                           const uint64_t* keys, const int64_t* n_dev, int64_t capacity_map, const double* mean, const double* info,
                           const uint8_t* valid, double voxel, int neighbors, int max_iteration, double eps_rot, double eps_trans,
                           double* T, double* fitness, double* score, int32_t* iterations, int32_t* status, double* T_trace,
                           double* eval_trace, double* sums_trace, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(ndt_register_shape_ok(n_src, n_pairs) && capacity_map >= 0 && capacity_map < (1ll << 31), EGONN_ERR_INVALID,
                "ndt_register: bad shape (n_src=%lld, capacity_map=%lld, both < 2^31; n_pairs=%d in [1, %d])", (long long)n_src,
                (long long)capacity_map, n_pairs, EGONN_MAX_BATCH);
  EGONN_REQUIRE(ndt_pos(voxel), EGONN_ERR_INVALID, "ndt_register: voxel must be finite and > 0");
  EGONN_REQUIRE(neighbors == 1 || neighbors == 7, EGONN_ERR_INVALID, "ndt_register: neighbors %d is neither 1 nor 7", neighbors);
  EGONN_REQUIRE(max_iteration >= 0 && max_iteration <= 100000, EGONN_ERR_INVALID, "ndt_register: max_iteration %d outside [0, 100000]",
                max_iteration);
  EGONN_REQUIRE(ndt_pos(eps_rot) && ndt_pos(eps_trans), EGONN_ERR_INVALID, "ndt_register: eps_rot and eps_trans must be finite and > 0");
  EGONN_REQUIRE(src_offsets && n_dev && T && fitness && score && iterations && status && scratch && (n_src == 0 || src) &&
                    (capacity_map == 0 || (keys && mean && info && valid)),
                EGONN_ERR_INVALID, "ndt_register: null pointer");
  const NdtSpan S = ndt_register_span(scratch, n_src, n_pairs);
  EGONN_TRY(span_check("ndt_register", scratch, scratch_bytes, S.total));
  hipStream_t st = (hipStream_t)stream;
  NdtPair* pairs = S.pairs;
  int32_t* wg0 = S.wg0;
  double* partial = S.partial;
  EGONN_TRY(pair_clear_traces(T_trace, eval_trace, 4, n_pairs, max_iteration, st));
  if (sums_trace)
    HIP_CHECK(hipMemsetAsync(sums_trace, 0, (size_t)n_pairs * ((size_t)max_iteration + 1) * NDT_NPART * sizeof(double), st));
  hipLaunchKernelGGL(ndt_setup_kernel, dim3((unsigned)cdiv(n_pairs, NDT_WG)), dim3(NDT_WG), 0, st, src_offsets, n_src, n_pairs, T_init,
                     pairs, wg0, T, fitness, score, iterations, status, T_trace, max_iteration);
  HIP_CHECK(hipGetLastError());
  if (n_src == 0) return EGONN_OK;                       // every pair is EMPTY
  const NdtLayer M = {keys, n_dev, capacity_map, mean, info, valid};
  const dim3 grid((unsigned)S.n_wg), one((unsigned)n_pairs);
  for (int k = 0; k <= max_iteration; ++k) {
    if (neighbors == 7) hipLaunchKernelGGL(ndt_eval_kernel<7>, grid, dim3(NDT_WG), 0, st, pairs, wg0, n_pairs, src, M, voxel, partial);
    else hipLaunchKernelGGL(ndt_eval_kernel<1>, grid, dim3(NDT_WG), 0, st, pairs, wg0, n_pairs, src, M, voxel, partial);
    hipLaunchKernelGGL(ndt_finish_kernel, one, dim3(64), 0, st, pairs, wg0, partial, k, max_iteration, eps_rot, eps_trans, T, fitness,
                       score, iterations, status, T_trace, eval_trace, sums_trace);
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
