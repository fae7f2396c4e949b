// Spectral geometric verification of keypoint correspondences on the device: a hypothesis-free alternative to the RANSAC of
// registration.hip, after spectral matching [Leordeanu & Hebert 2005] as PointDSC and SGV use it for exactly these operands.
// Per pair, with m correspondences (p_i, q_i) = (kp1[corr[i][0]], kp2[corr[i][1]]) converted exactly to fp64:
//
//   1. M_ij = max(0, 1 - d_ij^2 / d_thr^2), d_ij = | |p_i - p_j| - |q_i - q_j| |, M_ii = 0: how well correspondences i and j
//      preserve each other's distance.  Computed in fp64 (squared lengths as (dx*dx + dy*dy) + dz*dz, the quotient as a
//      product with the host's 1 / d_thr^2), stored rounded to fp32.
//   2. v = 1 / sqrt(m) in every component; `iterations` times: u = M v, stop if |u| = 0, else v = u / |u|.
//      eigenvalue = v^T M v.  u_i = sum_j M_ij v_j is one fp64 fma chain in ascending j; |u|^2 and v^T (M v) are sums over i by
//      a 64-lane xor butterfly (32, 16, .. 1) and then the waves' sums in ascending wave order.  No float atomics.
//   3. score = eigenvalue / (n_max - 1) (0 when n_max = 1).
//   4. seeds S = { i : v_i >= seed_ratio * max v }.
//   5. T0 = rigid fit of S; I = { i : |T0 p_i - q_i| < dist_th }; T = rigid fit of I; then pair_tail (pair_eval.h), the text
//      egonn_registration_finish ends with: the final evaluation under T (every source keypoint against its nearest target
//      keypoint) and the metrics.
//   6. m < 3: FEW_CORR.  M = 0 (|u| = 0 can only happen in the first iteration: M is symmetric, so M (M w) = 0 implies M w = 0),
//      |S| < 3, |I| < 3 or a degenerate fit: NO_MODEL.  Both: T = identity, 0 inliers.
//
// The rigid fit (spv_fit): centroids, then the centred cross-covariance S = sum (p - pm)(q - qm)^T and both scatter matrices,
// Horn's rotation of S (horn.h, the routine ICP uses), t = qm - R pm.  A point set is degenerate (coincident or collinear) when
// its scatter matrix C has e2(C) <= 1e-10 tr(C)^2, e2 = the sum of the principal 2 x 2 minors = l1 l2 + l1 l3 + l2 l3 of its
// eigenvalues: a set thinner than about 1e-5 of its length, which is where Horn's top eigenvalue stops being simple.
//
// One workgroup per pair, one lane per correspondence (= per row of M); a lane builds its own row and is the only reader of
// it, so M needs no barrier.  n_max <= 128: M in LDS as fp32, row stride 129 words (the 32 lanes of an LDS access group hit 32
// banks), 66 KB + 12 KB of points and vectors = 78 KB, two workgroups of 128 lanes per CU.  n_max > 128: a full matrix does not
// fit, so each of at most 512 workgroups owns an n_max x n_max fp32 slab of the caller's scratch, stored column-major (lane i
// reads M_ij at j * n_max + i: a coalesced line per j) and walks the pairs b, b + 512, ...; a pair's arithmetic is the same in
// both forms and does not depend on the workgroup that runs it.
#include "../../include/egonn_hip.h"
#include "common.h"
#include "horn.h"
#include "pair_eval.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int SPV_LDS_N = 128;      // largest n_max whose M lives in LDS
static constexpr int SPV_SLABS = 512;      // workgroups (= slabs of scratch) of the form for larger n_max
static constexpr int SPV_NRED = 21;        // widest reduction: 9 cross-covariance + 2 x 6 scatter entries
static constexpr double SPV_DEGEN = 1e-10;

struct SpvArgs {
  PairIn in;
  int n_pairs, iterations;
  double inv_thr2, seed_ratio;
  float* slab;
  double *eigenvalue, *score, *weights;
  int32_t* n_seeds;
  PairOut out;
};

template <int NT>
struct SpvShared {
  double c[6][NT];             // the correspondences' points: source x, y, z, target x, y, z
  double v[NT];
  double red[SPV_NRED][NT / 64];
  PairTailShared<NT> tail;
};

// x[k] summed over the workgroup, for k < K: butterfly inside a wave, then the waves in ascending order.  Valid in every lane.
template <int NT, int K>
__device__ static inline void spv_sum(double* x, double (*red)[NT / 64]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x[k] += __shfl_xor(x[k], o, 64);
  __syncthreads();   // the readers of the reduction before this one are done
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][w] = x[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = red[k][0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) s += red[k][i];
    x[k] = s;
  }
}

template <int NT>
__device__ static inline double spv_max(double x, double (*red)[NT / 64]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
  __syncthreads();
  if (lane == 0) red[0][w] = x;
  __syncthreads();
  double s = red[0][0];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) s = fmax(s, red[0][i]);
  return s;
}

// e2(C) > SPV_DEGEN tr(C)^2 for the scatter matrix C = (c00, c01, c02, c11, c12, c22); false for NaN as well
__device__ static inline bool spv_spread(const double* c) {
  const double tr = c[0] + c[3] + c[5];
  const double e2 = (c[0] * c[3] - c[1] * c[1]) + (c[0] * c[5] - c[2] * c[2]) + (c[3] * c[5] - c[4] * c[4]);
  return e2 > SPV_DEGEN * (tr * tr);
}

// Least-squares rigid transform (no scale, det +1) of the correspondences whose lane passes `in`.  Called by the whole
// workgroup; the result (and the return value) is the same in every lane.  False: fewer than 3 members or a degenerate set.
template <int NT>
__device__ static bool spv_fit(SpvShared<NT>& sh, bool in, double* R, double* tv) {
  const int t = threadIdx.x;
  double p[3], q[3], a[7];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = in ? sh.c[k][t] : 0.0, q[k] = in ? sh.c[3 + k][t] : 0.0;
  a[0] = in ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) a[1 + k] = p[k], a[4 + k] = q[k];
  spv_sum<NT, 7>(a, sh.red);
  if (!(a[0] >= 3.0)) return false;
  double pm[3], qm[3], b[SPV_NRED];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    pm[k] = a[1 + k] / a[0], qm[k] = a[4 + k] / a[0];
    p[k] = in ? p[k] - pm[k] : 0.0, q[k] = in ? q[k] - qm[k] : 0.0;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) b[r * 3 + c] = p[r] * q[c];
  b[9] = p[0] * p[0], b[10] = p[0] * p[1], b[11] = p[0] * p[2], b[12] = p[1] * p[1], b[13] = p[1] * p[2], b[14] = p[2] * p[2];
  b[15] = q[0] * q[0], b[16] = q[0] * q[1], b[17] = q[0] * q[2], b[18] = q[1] * q[1], b[19] = q[1] * q[2], b[20] = q[2] * q[2];
  spv_sum<NT, SPV_NRED>(b, sh.red);
  if (!spv_spread(b + 9) || !spv_spread(b + 15)) return false;
  double S[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) S[r][c] = b[r * 3 + c];
  horn_rotation(S, R);
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    tv[r] = qm[r] - (R[r * 3] * pm[0] + R[r * 3 + 1] * pm[1] + R[r * 3 + 2] * pm[2]);
    ok = ok && fabs(tv[r]) < INFINITY && fabs(R[r * 3]) < INFINITY && fabs(R[r * 3 + 1]) < INFINITY && fabs(R[r * 3 + 2]) < INFINITY;
  }
  return ok;
}

// One pair by the whole workgroup.  row = this lane's row of M, element j at row[j * rs].
template <int NT>
__device__ static void spv_pair(const SpvArgs& a, int p, float* __restrict__ row, int rs, SpvShared<NT>& sh) {
  const int t = threadIdx.x, n_max = a.in.n_max;
  const PairView pv = pair_view(a.in, p);
  const int nc = pv.nc;
  const double v0 = nc > 0 ? 1.0 / sqrt((double)nc) : 0.0;
  sh.v[t] = t < nc ? v0 : 0.0;
  const int st = pair_load_corr_status(pv, sh.c);   // the correspondences' points; its barrier covers v as well

  // 1. this lane's row of M
  double pc[6] = {0, 0, 0, 0, 0, 0};
  if (t < nc) {
#pragma unroll
    for (int k = 0; k < 6; ++k) pc[k] = sh.c[k][t];
    for (int j = 0; j < nc; ++j) {   // every lane reads the same column's point: LDS broadcast
      const double ax = pc[0] - sh.c[0][j], ay = pc[1] - sh.c[1][j], az = pc[2] - sh.c[2][j];
      const double bx = pc[3] - sh.c[3][j], by = pc[4] - sh.c[4][j], bz = pc[5] - sh.c[5][j];
      const double d = sqrt((ax * ax + ay * ay) + az * az) - sqrt((bx * bx + by * by) + bz * bz);
      const double x = 1.0 - (d * d) * a.inv_thr2;
      row[(size_t)j * rs] = (j != t && x > 0.0) ? (float)x : 0.f;
    }
  }

  // 2. power iteration
  bool zero = false;
  double u = 0.0;
  for (int it = 0; it <= a.iterations; ++it) {   // the last round only evaluates u = M v for the eigenvalue
    u = 0.0;
    if (t < nc)
      for (int j = 0; j < nc; ++j) u = fma((double)row[(size_t)j * rs], sh.v[j], u);
    if (it == a.iterations) break;
    double n2 = u * u;
    spv_sum<NT, 1>(&n2, sh.red);
    if (!(n2 > 0.0)) {
      zero = true;
      break;
    }
    sh.v[t] = u / sqrt(n2);
    __syncthreads();
  }
  const double vt = sh.v[t];
  double lam = zero ? 0.0 : vt * u;
  spv_sum<NT, 1>(&lam, sh.red);
  const double vmax = spv_max<NT>(vt, sh.red);

  // 4. seeds, 5. two fits
  const bool seed = t < nc && vt >= a.seed_ratio * vmax;
  const int n_seeds = __syncthreads_count(seed);
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tf[3] = {0, 0, 0};
  bool model = false;
  if (nc >= 3 && !zero) {
    double R0[9], t0[3];
    if (spv_fit<NT>(sh, seed, R0, t0)) {
      const bool in = t < nc && pair_res2(R0, t0, pc[0], pc[1], pc[2], pc[3], pc[4], pc[5]) < a.in.th2;
      model = spv_fit<NT>(sh, in, R0, t0);
      if (model) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = R0[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tf[k] = t0[k];
      }
    }
  }
  if (t == 0) {
    if (a.eigenvalue) a.eigenvalue[p] = lam;
    if (a.score) a.score[p] = n_max > 1 ? lam / (double)(n_max - 1) : 0.0;
    if (a.n_seeds) a.n_seeds[p] = n_seeds;
  }
  if (a.weights && t < n_max) a.weights[(size_t)p * n_max + t] = vt;
  pair_tail<NT>(a.in, a.out, p, pv, true, model, R, tf, st, sh.tail);
}

template <int NT, bool LDS_M>
__global__ __launch_bounds__(NT) void spectral_kernel(const SpvArgs a) {
  extern __shared__ float s_m[];   // LDS_M: NT rows of NT + 1 words
  __shared__ SpvShared<NT> sh;
  const int t = threadIdx.x;
  float* row = LDS_M ? s_m + t * (NT + 1) : a.slab + (size_t)blockIdx.x * a.in.n_max * a.in.n_max + t;
  const int rs = LDS_M ? 1 : a.in.n_max;
  for (int p = blockIdx.x; p < a.n_pairs; p += gridDim.x) {
    spv_pair<NT>(a, p, row, rs, sh);
    __syncthreads();   // the next pair overwrites the shared arrays
  }
}

}  // namespace egonn

using namespace egonn;

API int64_t egonn_spectral_verify_scratch_bytes(int n_pairs, int n_max) {
  if (n_pairs < 0 || n_pairs > KP_MAX_PAIRS || n_max < 1 || n_max > KP_MAX_N) return -1;
  if (n_max <= SPV_LDS_N) return 0;
  return (int64_t)(n_pairs < SPV_SLABS ? n_pairs : SPV_SLABS) * n_max * n_max * (int64_t)sizeof(float);
}

API int egonn_spectral_verify(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2, const int32_t* corr,
                              const int32_t* n_corr, int n_pairs, int n_max, double d_thr, int iterations, double seed_ratio,
                              double dist_th, const double* T_gt, double repeat_th, void* scratch, int64_t scratch_bytes,
                              double* eigenvalue, double* score, double* weights, int32_t* n_seeds, double* T, int32_t* inliers,
                              double* fitness, double* inlier_rmse, int32_t* corr_set, double* rte, double* rre, int32_t* success,
                              double* repeatability, int32_t* status, void* stream) {
  EGONN_TRY(reg_check_shape("spectral_verify", n_pairs, n_max));
  EGONN_REQUIRE(kp1 && kp2 && n1 && n2 && corr && n_corr, EGONN_ERR_INVALID, "spectral_verify: null pointer");
  EGONN_REQUIRE(d_thr > 0.0 && d_thr < 1e18, EGONN_ERR_INVALID, "spectral_verify: bad consistency threshold d_thr");
  EGONN_REQUIRE(iterations >= 1, EGONN_ERR_INVALID, "spectral_verify: iterations %d must be positive", iterations);
  EGONN_REQUIRE(seed_ratio > 0.0 && seed_ratio <= 1.0, EGONN_ERR_INVALID, "spectral_verify: seed_ratio must be in (0, 1]");
  EGONN_TRY(reg_check_threshold("spectral_verify", "distance", dist_th, false));
  if (T_gt) EGONN_TRY(reg_check_threshold("spectral_verify", "repeatability", repeat_th, true));
  const int64_t need = egonn_spectral_verify_scratch_bytes(n_pairs, n_max);
  EGONN_REQUIRE(need == 0 || (scratch && scratch_bytes >= need && ((uintptr_t)scratch & 7) == 0), EGONN_ERR_INVALID,
                "spectral_verify: scratch needs %lld bytes, 8-byte aligned", (long long)need);
  if (n_pairs == 0) return EGONN_OK;
  SpvArgs a;
  a.in = PairIn{kp1, kp2, n1, n2, corr, n_corr, n_max, dist_th * dist_th, repeat_th * repeat_th, T_gt};
  a.n_pairs = n_pairs, a.iterations = iterations, a.inv_thr2 = 1.0 / (d_thr * d_thr), a.seed_ratio = seed_ratio;
  a.slab = (float*)scratch, a.eigenvalue = eigenvalue, a.score = score, a.weights = weights, a.n_seeds = n_seeds;
  a.out = PairOut{T, inliers, fitness, inlier_rmse, corr_set, rte, rre, success, repeatability, status};
  if (n_max <= SPV_LDS_N) {
    constexpr size_t lds = (size_t)SPV_LDS_N * (SPV_LDS_N + 1) * sizeof(float);
    static AttrOnce attr;
    if (attr.need()) {
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&spectral_kernel<SPV_LDS_N, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   // beside 12 KB of static LDS
      attr.mark();
    }
    hipLaunchKernelGGL((spectral_kernel<SPV_LDS_N, true>), dim3((unsigned)n_pairs), dim3(SPV_LDS_N), lds, (hipStream_t)stream, a);
  } else {
    const unsigned grid = (unsigned)(n_pairs < SPV_SLABS ? n_pairs : SPV_SLABS);
    hipLaunchKernelGGL((spectral_kernel<KP_MAX_N, false>), dim3(grid), dim3(KP_MAX_N), 0, (hipStream_t)stream, a);
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
