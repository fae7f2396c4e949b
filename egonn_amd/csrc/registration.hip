// 6-DoF registration of two keypoint sets on the device: the consumer of the LOCAL half of the descriptor path
// (reference eval/evaluate.py: get_ransac_result :381-399, ransac_fn :296-306, calculate_repeatability :402-411 and the
// RRE / RTE / success bookkeeping :239-259).  The reference hands the step to Open3D's
// registration_ransac_based_on_feature_matching (mutual_filter, max distance 0.5, point-to-point without scale,
// ransac_n = 3, checkers EdgeLength(0.8) + Distance(0.5), criteria (10000, 0.999)).  Open3D is not part of the reference
// tree, so what follows restates its documented behaviour [recall], batched over P independent (query, candidate) pairs:
//
//   1. egonn_match_mutual (match.hip)  the mutual nearest neighbours of the two descriptor sets, compacted in ascending i.
//   2. reg_ransac_kernel  hypothesis t = 0 .. H-1, one lane each (see reg_hypothesis below); per workgroup the best
//                         (inliers, err2, t) goes to scratch.
//   3. reg_finish_kernel  best over the workgroups' records, the winner's transform again (same code, same bits), then
//                         pair_tail (pair_eval.h, shared with spectral.hip): the final evaluation over ALL source
//                         keypoints and the metrics against a caller's T_gt.
//
// Two deliberate differences from Open3D: (a) Open3D stops early by its 0.999 confidence rule, here every one of the H
// hypotheses is evaluated (a superset of what Open3D tries); (b) Open3D draws from a thread-dependent generator, here a
// draw is a pure function of (seed, pair id, t, slot), so the result is reproducible bit for bit and does not depend on the
// batch a pair sits in nor on how the hypotheses are spread over workgroups.
//
// The draw (reg_draw): with 64-bit wrapping arithmetic
//       ctr = (pair_id << 34) | (t << 2) | slot                     pair_id < 2^30, t < 2^31, slot in {0, 1, 2}
//       z   = seed + 0x9E3779B97F4A7C15 * (ctr + 1)                 (the state of splitmix64(seed) after ctr + 1 steps)
//       z   = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//       z   = (z ^ (z >> 27)) * 0x94D049BB133111EB
//       z   =  z ^ (z >> 31)
//       draw = ((z >> 32) * n_corr) >> 32                           (multiply-high of the upper word, in [0, n_corr))
//
// Best rule: most inliers (= highest fitness, n_corr is common), then smallest sum of squared inlier distances err2
// (= lowest rmse at equal inliers; compared before the square root, which is the finer order), then lowest t.  It is a
// total order, so the two-stage reduction gives the same winner under every chunking; there are no float atomics.
//
// All geometry is fp64 with contraction off: every operation below is the IEEE operation that is written, so the
// transform the finish kernel recomputes is the one the hot loop scored.
#include "../../include/egonn_hip.h"
#include "common.h"
#include "pair_eval.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int REG_WG = 256;       // lanes = hypotheses per workgroup of the hot loop
static constexpr double REG_EDGE2 = 0.8 * 0.8;   // CorrespondenceCheckerBasedOnEdgeLength(0.8), on squared lengths
static constexpr double REG_DEGEN2 = 1e-6;       // |e1 x e2|^2 <= 1e-6 |e1|^2 |e2|^2  <=>  |e1 x e2| <= 1e-3 |e1| |e2|

struct RegPartial {   // one workgroup's best hypothesis
  int32_t cnt;        // inliers, -1 = none accepted in the chunk
  int32_t t;
  double err2;
};

__host__ __device__ static inline uint32_t reg_draw(uint64_t seed, uint32_t pair_id, uint32_t t, uint32_t slot, uint32_t n) {
  const uint64_t ctr = ((uint64_t)pair_id << 34) | ((uint64_t)t << 2) | (uint64_t)slot;
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (ctr + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (uint32_t)(((z >> 32) * (uint64_t)n) >> 32);
}

__device__ static inline bool reg_better(int c1, double e1, int t1, int c2, double e2, int t2) {
  return c1 > c2 || (c1 == c2 && (e1 < e2 || (e1 == e2 && t1 < t2)));
}

// ------------------------------------------------------------------ shared geometry
// RANSAC works on centred coordinates: the correspondences' points that pair_load_corr (pair_eval.h) put into s_c, centred on
// the centroids of their source / target points (sums in ascending correspondence order by one lane per coordinate: a fixed
// order).  s_cent[0..2] = the source centroid, s_cent[3..5] = the target's.  Called behind the barrier that follows the load.
__device__ static void reg_centre(double (*s_c)[KP_MAX_N], int nc, double* s_cent) {
  const int t = threadIdx.x;
  if (t < 6) {
    double s = 0.0;
    for (int c = 0; c < nc; ++c) s += s_c[t][c];
    s_cent[t] = nc > 0 ? s / (double)nc : 0.0;
  }
  __syncthreads();
  if (t < nc) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s_c[k][t] -= s_cent[k];
  }
  __syncthreads();
}

__device__ static inline void reg_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ static inline double reg_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// One hypothesis on the centred correspondences in LDS.  Returns 0 = accepted (R row-major and tv, in centred coordinates),
// -1 = degenerate draw (a repeated correspondence, or a source or target triangle with |e1 x e2| <= 1e-3 |e1| |e2|),
// -2 = edge-length check (every edge: |s_a - s_b| >= 0.8 |t_a - t_b| and the converse; on squared lengths),
// -3 = distance check (a transformed sample point farther than dist_th from its target).
//
// The rigid transform of three point pairs in closed form: the centred triples span a plane each, so the cross-covariance
// has rank 2 and the least-squares rotation (Kabsch / Umeyama with the reflection correction) maps the source plane onto
// the target plane.  In orthonormal frames (f1, f2, ns) / (g1, g2, nt) of the two planes it is the 2 x 2 orthogonal factor
// O of A = sum_k p_k q_k^T (p, q = in-plane coordinates) that maximises tr(O A^T): the rotation by atan2(a12 - a21, a11 + a22)
// when det A >= 0, else the reflection by atan2(a12 + a21, a11 - a22), and the normal maps to det(O) times the normal, which
// makes det R = +1.  No iteration, no square root of a small difference.
__device__ static int reg_hypothesis(const double (*s_c)[KP_MAX_N], int nc, uint64_t seed, uint32_t pid, uint32_t t,
                                     double th2, double* R, double* tv) {
  const int ia = (int)reg_draw(seed, pid, t, 0, (uint32_t)nc), ib = (int)reg_draw(seed, pid, t, 1, (uint32_t)nc),
            ic = (int)reg_draw(seed, pid, t, 2, (uint32_t)nc);
  if (ia == ib || ia == ic || ib == ic) return -1;
  const int idx[3] = {ia, ib, ic};
  double S[3][3], Q[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      S[k][c] = s_c[c][idx[k]];
      Q[k][c] = s_c[3 + c][idx[k]];
    }
  double e1[3], e2[3], e3[3], f1[3], f2[3], f3[3], ns[3], nt[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    e1[c] = S[1][c] - S[0][c];
    e2[c] = S[2][c] - S[0][c];
    e3[c] = S[2][c] - S[1][c];
    f1[c] = Q[1][c] - Q[0][c];
    f2[c] = Q[2][c] - Q[0][c];
    f3[c] = Q[2][c] - Q[1][c];
  }
  reg_cross(e1, e2, ns);
  reg_cross(f1, f2, nt);
  const double le1 = reg_dot(e1, e1), le2 = reg_dot(e2, e2), le3 = reg_dot(e3, e3);
  const double lf1 = reg_dot(f1, f1), lf2 = reg_dot(f2, f2), lf3 = reg_dot(f3, f3);
  const double ns2 = reg_dot(ns, ns), nt2 = reg_dot(nt, nt);
  if (!(ns2 > REG_DEGEN2 * le1 * le2) || !(nt2 > REG_DEGEN2 * lf1 * lf2)) return -1;
  if (!(le1 >= REG_EDGE2 * lf1 && lf1 >= REG_EDGE2 * le1 && le2 >= REG_EDGE2 * lf2 && lf2 >= REG_EDGE2 * le2 &&
        le3 >= REG_EDGE2 * lf3 && lf3 >= REG_EDGE2 * le3))
    return -2;
  // plane frames
  double fs1[3], fs2[3], gt1[3], gt2[3];
  const double ie = 1.0 / sqrt(le1), ig = 1.0 / sqrt(lf1), ins = 1.0 / sqrt(ns2), int_ = 1.0 / sqrt(nt2);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    fs1[c] = e1[c] * ie;
    gt1[c] = f1[c] * ig;
    ns[c] *= ins;
    nt[c] *= int_;
  }
  reg_cross(ns, fs1, fs2);
  reg_cross(nt, gt1, gt2);
  double cs[3], ct[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    cs[c] = (S[0][c] + S[1][c] + S[2][c]) / 3.0;
    ct[c] = (Q[0][c] + Q[1][c] + Q[2][c]) / 3.0;
  }
  double a11 = 0.0, a12 = 0.0, a21 = 0.0, a22 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double ps[3], qs[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ps[c] = S[k][c] - cs[c];
      qs[c] = Q[k][c] - ct[c];
    }
    const double p0 = reg_dot(ps, fs1), p1 = reg_dot(ps, fs2), q0 = reg_dot(qs, gt1), q1 = reg_dot(qs, gt2);
    a11 += p0 * q0;
    a12 += p0 * q1;
    a21 += p1 * q0;
    a22 += p1 * q1;
  }
  const double cr = a11 + a22, sr = a12 - a21, cf = a11 - a22, sf = a12 + a21;
  const double vr = cr * cr + sr * sr, vf = cf * cf + sf * sf;
  double o11, o12, o21, o22, det;
  if (vr >= vf) {
    if (!(vr > 0.0)) return -1;
    const double h = 1.0 / sqrt(vr), c = cr * h, s = sr * h;
    o11 = c, o12 = -s, o21 = s, o22 = c, det = 1.0;
  } else {
    const double h = 1.0 / sqrt(vf), c = cf * h, s = sf * h;
    o11 = c, o12 = s, o21 = s, o22 = -c, det = -1.0;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      R[r * 3 + c] = o11 * gt1[r] * fs1[c] + o12 * gt1[r] * fs2[c] + o21 * gt2[r] * fs1[c] + o22 * gt2[r] * fs2[c] +
                     det * nt[r] * ns[c];
#pragma unroll
  for (int r = 0; r < 3; ++r) tv[r] = ct[r] - (R[r * 3] * cs[0] + R[r * 3 + 1] * cs[1] + R[r * 3 + 2] * cs[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (!(pair_res2(R, tv, S[k][0], S[k][1], S[k][2], Q[k][0], Q[k][1], Q[k][2]) <= th2)) return -3;
  return 0;
}

// workgroup-wide best of (cnt, err2, t) under reg_better; the result is valid in every lane
__device__ static void reg_block_best(int& cnt, double& err2, int& bt, int* s_cnt, int* s_t, double* s_e) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(cnt, o, 64), ot = __shfl_xor(bt, o, 64);
    const double oe = __shfl_xor(err2, o, 64);
    if (reg_better(oc, oe, ot, cnt, err2, bt)) cnt = oc, err2 = oe, bt = ot;
  }
  __syncthreads();
  if (lane == 0) s_cnt[w] = cnt, s_t[w] = bt, s_e[w] = err2;
  __syncthreads();
  cnt = s_cnt[0], bt = s_t[0], err2 = s_e[0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (reg_better(s_cnt[k], s_e[k], s_t[k], cnt, err2, bt)) cnt = s_cnt[k], err2 = s_e[k], bt = s_t[k];
}

// ------------------------------------------------------------------ 2. the hot loop: one lane = one hypothesis
__global__ __launch_bounds__(REG_WG) void reg_ransac_kernel(const float* __restrict__ kp1, const float* __restrict__ kp2,
                                                            const int32_t* __restrict__ n1, const int32_t* __restrict__ n2,
                                                            const int32_t* __restrict__ corr,
                                                            const int32_t* __restrict__ n_corr,
                                                            const int32_t* __restrict__ pair_id, int n_max, int H, int chunks,
                                                            uint64_t seed, double th2, RegPartial* __restrict__ partial,
                                                            int32_t* __restrict__ hyp_count, double* __restrict__ hyp_err2) {
  __shared__ double s_c[6][KP_MAX_N];   // 12 KB
  __shared__ double s_cent[6];
  __shared__ int s_cnt[4], s_t[4];
  __shared__ double s_e[4];
  const int p = blockIdx.x / chunks, chunk = blockIdx.x % chunks, t = chunk * REG_WG + (int)threadIdx.x;
  const int m1 = clipi(n1[p], n_max), m2 = clipi(n2[p], n_max);
  const int nc = pair_nc(m1, m2, n_corr[p], n_max);
  pair_load_corr(kp1 + (size_t)p * n_max * 3, kp2 + (size_t)p * n_max * 3, m1, m2, corr + (size_t)p * n_max * 2, nc, s_c);
  __syncthreads();
  reg_centre(s_c, nc, s_cent);
  const uint32_t pid = pair_id ? (uint32_t)pair_id[p] & 0x3fffffffu : (uint32_t)p;
  int cnt = -1, code = -1;
  double err2 = 0.0;
  if (t < H && nc >= 3) {
    double R[9], tv[3];
    code = reg_hypothesis(s_c, nc, seed, pid, (uint32_t)t, th2, R, tv);
    if (code == 0) {
      cnt = 0;
      for (int c = 0; c < nc; ++c) {   // every lane reads the same correspondence: LDS broadcast
        const double d2 = pair_res2(R, tv, s_c[0][c], s_c[1][c], s_c[2][c], s_c[3][c], s_c[4][c], s_c[5][c]);
        if (d2 < th2) {
          ++cnt;
          err2 += d2;
        }
      }
    }
  }
  if (t < H) {
    if (hyp_count) hyp_count[(size_t)p * H + t] = code == 0 ? cnt : code;
    if (hyp_err2) hyp_err2[(size_t)p * H + t] = err2;
  }
  int bt = t < H ? t : 0x7fffffff;
  reg_block_best(cnt, err2, bt, s_cnt, s_t, s_e);
  if (threadIdx.x == 0) {
    RegPartial r;
    r.cnt = cnt, r.t = bt, r.err2 = err2;
    partial[(size_t)p * chunks + chunk] = r;
  }
}

// ------------------------------------------------------------------ 3. best hypothesis, then the tail of pair_eval.h
struct RegFinishArgs {
  PairIn in;
  const int32_t* pair_id;
  int H, chunks;
  uint64_t seed;
  const RegPartial* partial;
  int32_t* best_t;
  PairOut out;
};

__global__ __launch_bounds__(REG_WG) void reg_finish_kernel(const RegFinishArgs a) {
  __shared__ double s_c[6][KP_MAX_N];
  __shared__ double s_cent[6];
  __shared__ int s_cnt[4], s_t[4];
  __shared__ double s_e[4];
  __shared__ alignas(16) PairTailShared<REG_WG> s_tail;   // the search reads two targets per 128-bit LDS load
  const int p = blockIdx.x, t = threadIdx.x;
  const PairView v = pair_view(a.in, p);
  int st = v.st;

  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tf[3] = {0, 0, 0};   // T = identity unless a hypothesis was accepted
  int bt = -1;
  if (v.cp) {
    const int nc = v.nc;
    st = pair_load_corr_status(v, s_c);   // ends in a barrier
    reg_centre(s_c, nc, s_cent);
    int cnt = -1, ct = 0x7fffffff;
    double e = 0.0;
    for (int c = t; c < a.chunks; c += REG_WG) {
      const RegPartial r = a.partial[(size_t)p * a.chunks + c];
      if (reg_better(r.cnt, r.err2, r.t, cnt, e, ct)) cnt = r.cnt, e = r.err2, ct = r.t;
    }
    reg_block_best(cnt, e, ct, s_cnt, s_t, s_e);
    if (nc >= 3 && cnt > 0 && ct >= 0 && ct < a.H) {
      const uint32_t pid = a.pair_id ? (uint32_t)a.pair_id[p] & 0x3fffffffu : (uint32_t)p;
      double tv[3];
      if (reg_hypothesis(s_c, nc, a.seed, pid, (uint32_t)ct, a.in.th2, R, tv) == 0) {   // every lane: the same bits
        bt = ct;
#pragma unroll
        for (int r = 0; r < 3; ++r)   // centred -> caller's coordinates
          tf[r] = s_cent[3 + r] + tv[r] - (R[r * 3] * s_cent[0] + R[r * 3 + 1] * s_cent[1] + R[r * 3 + 2] * s_cent[2]);
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
      }
    }
    if (t == 0 && a.best_t) a.best_t[p] = bt;
  }
  pair_tail<REG_WG>(a.in, a.out, p, v, v.cp != nullptr, bt >= 0, R, tf, st, s_tail);
}

int reg_check_shape(const char* who, int P, int n_max) {
  EGONN_REQUIRE(P >= 0 && P <= KP_MAX_PAIRS && n_max >= 1 && n_max <= KP_MAX_N, EGONN_ERR_INVALID,
                "%s: bad shape (P=%d, n_max=%d; n_max <= %d)", who, P, n_max, KP_MAX_N);
  return EGONN_OK;
}

// dist_th in (0, 1e18), repeat_th in [0, 1e18): the kernels compare with the square
int reg_check_threshold(const char* who, const char* what, double th, bool zero_ok) {
  EGONN_REQUIRE((th > 0.0 || (zero_ok && th == 0.0)) && th < 1e18, EGONN_ERR_INVALID, "%s: bad %s threshold", who, what);
  return EGONN_OK;
}

}  // namespace egonn

using namespace egonn;

API int64_t egonn_registration_scratch_bytes(int n_pairs, int n_max, int n_hypotheses) {
  if (n_pairs < 0 || n_max < 1 || n_max > KP_MAX_N || n_hypotheses <= 0) return -1;
  return (int64_t)n_pairs * cdiv(n_hypotheses, REG_WG) * (int64_t)sizeof(RegPartial);
}

API int egonn_ransac_pairs(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2, const int32_t* corr,
                           const int32_t* n_corr, const int32_t* pair_id, int n_pairs, int n_max, int n_hypotheses,
                           uint64_t seed, double dist_th, void* scratch, int64_t scratch_bytes, int32_t* hyp_count,
                           double* hyp_err2, void* stream) {
  EGONN_TRY(reg_check_shape("ransac_pairs", n_pairs, n_max));
  EGONN_REQUIRE(n_hypotheses > 0, EGONN_ERR_INVALID, "ransac_pairs: n_hypotheses %d must be positive", n_hypotheses);
  EGONN_REQUIRE(kp1 && kp2 && n1 && n2 && corr && n_corr && scratch, EGONN_ERR_INVALID, "ransac_pairs: null pointer");
  EGONN_TRY(reg_check_threshold("ransac_pairs", "distance", dist_th, false));
  const int64_t chunks = cdiv(n_hypotheses, REG_WG);
  EGONN_REQUIRE(scratch_bytes >= egonn_registration_scratch_bytes(n_pairs, n_max, n_hypotheses) &&
                    ((uintptr_t)scratch & 7) == 0,
                EGONN_ERR_INVALID, "ransac_pairs: scratch needs %lld bytes, 8-byte aligned",
                (long long)egonn_registration_scratch_bytes(n_pairs, n_max, n_hypotheses));
  EGONN_REQUIRE((int64_t)n_pairs * chunks < (1ll << 31), EGONN_ERR_INVALID, "ransac_pairs: %d pairs x %d hypotheses is too large a grid",
                n_pairs, n_hypotheses);
  if (n_pairs == 0) return EGONN_OK;
  hipLaunchKernelGGL(reg_ransac_kernel, dim3((unsigned)(n_pairs * chunks)), dim3(REG_WG), 0, (hipStream_t)stream, kp1, kp2, n1, n2,
                     corr, n_corr, pair_id, n_max, n_hypotheses, (int)chunks, seed, dist_th * dist_th, (RegPartial*)scratch,
                     hyp_count, hyp_err2);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_registration_finish(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2, const int32_t* corr,
                                  const int32_t* n_corr, const int32_t* pair_id, int n_pairs, int n_max, int n_hypotheses,
                                  uint64_t seed, double dist_th, const void* scratch, int64_t scratch_bytes, const double* T_gt,
                                  double repeat_th, double* T, int32_t* inliers, double* fitness, double* inlier_rmse,
                                  int32_t* corr_set, int32_t* best_t, double* rte, double* rre, int32_t* success,
                                  double* repeatability, int32_t* status, void* stream) {
  EGONN_TRY(reg_check_shape("registration_finish", n_pairs, n_max));
  EGONN_REQUIRE(kp1 && kp2 && n1 && n2, EGONN_ERR_INVALID, "registration_finish: null pointer");
  int chunks = 0;
  if (corr) {
    EGONN_REQUIRE(n_hypotheses > 0, EGONN_ERR_INVALID, "registration_finish: n_hypotheses %d must be positive", n_hypotheses);
    EGONN_REQUIRE(n_corr && scratch && T && inliers && fitness && inlier_rmse, EGONN_ERR_INVALID,
                  "registration_finish: null pointer");
    EGONN_TRY(reg_check_threshold("registration_finish", "distance", dist_th, false));
    EGONN_REQUIRE(scratch_bytes >= egonn_registration_scratch_bytes(n_pairs, n_max, n_hypotheses) &&
                      ((uintptr_t)scratch & 7) == 0,
                  EGONN_ERR_INVALID, "registration_finish: scratch needs %lld bytes, 8-byte aligned",
                  (long long)egonn_registration_scratch_bytes(n_pairs, n_max, n_hypotheses));
    chunks = (int)cdiv(n_hypotheses, REG_WG);
  } else {
    EGONN_REQUIRE(T_gt && repeatability, EGONN_ERR_INVALID,
                  "registration_finish: without correspondences only the T_gt metrics are computed: T_gt and repeatability needed");
  }
  if (T_gt) EGONN_TRY(reg_check_threshold("registration_finish", "repeatability", repeat_th, true));
  if (n_pairs == 0) return EGONN_OK;
  RegFinishArgs a;
  a.in = PairIn{kp1, kp2, n1, n2, corr, n_corr, n_max, dist_th * dist_th, repeat_th * repeat_th, T_gt};
  a.pair_id = pair_id, a.H = n_hypotheses, a.chunks = chunks, a.seed = seed, a.partial = (const RegPartial*)scratch, a.best_t = best_t;
  a.out = PairOut{T, inliers, fitness, inlier_rmse, corr_set, rte, rre, success, repeatability, status};
  hipLaunchKernelGGL(reg_finish_kernel, dim3((unsigned)n_pairs), dim3(REG_WG), 0, (hipStream_t)stream, a);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
