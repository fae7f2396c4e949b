// What follows a model of one keypoint pair, shared by the RANSAC finish (registration.hip) and the spectral verification
// (spectral.hip): the operands and outputs both entry points have in common, the clamped load of the correspondences' points with
// the status bits it decides, the residual |R s + t - q|^2, and the tail: final evaluation over ALL source keypoints under T,
// the 4 x 4 write, the metrics against a caller's T_gt (reference eval/evaluate.py: calculate_repeatability :402-411, the
// RRE / RTE / success bookkeeping :239-259) and the status word.  Both methods rank by `inliers` (egonn_pick_candidates), so
// there is one text for it.  All of it is fp64 with contraction off: every operation is the IEEE operation that is written.
#pragma once

#include "../../include/egonn_hip.h"
#include "common.h"
#include "pose_math.h"      // se3_store only: the arithmetic there is not this file's (contraction)

#pragma clang fp contract(off)

namespace egonn {

static constexpr double PAIR_RTE_MAX_M = 2.0;     // success: rte <= 2 m and rre <= 5 degrees (eval/evaluate.py:253)
static constexpr double PAIR_RRE_MAX_DEG = 5.0;

struct PairIn {    // operands, P pairs padded to n_max rows; corr == nullptr: no correspondences were given (T_gt metrics only)
  const float *kp1, *kp2;
  const int32_t *n1, *n2, *corr, *n_corr;
  int n_max;
  double th2, rth2;     // dist_th^2, repeat_th^2
  const double* T_gt;   // (P,4,4) or nullptr
};

struct PairOut {   // per-pair outputs; a null one is not written
  double* T;
  int32_t* inliers;
  double *fitness, *rmse;
  int32_t* corr_set;
  double *rte, *rre;
  int32_t* success;
  double* repeatability;
  int32_t* status;
};

struct PairView {       // pair p of a PairIn
  const float *k1, *k2;
  const int32_t* cp;    // its rows of corr, nullptr when none were given
  int m1, m2, nc;       // counts clipped to n_max; nc = 0 when a side is empty
  int st;               // EGONN_REG_STATUS_CLIPPED when a count was clipped
};

__device__ static inline int pair_nc(int m1, int m2, int nc_raw, int n_max) { return (m1 == 0 || m2 == 0) ? 0 : clipi(nc_raw, n_max); }

__device__ static inline PairView pair_view(const PairIn& in, int p) {
  PairView v;
  const int r1 = in.n1[p], r2 = in.n2[p], rc = in.corr ? in.n_corr[p] : 0;
  v.m1 = clipi(r1, in.n_max), v.m2 = clipi(r2, in.n_max);
  v.nc = in.corr ? pair_nc(v.m1, v.m2, rc, in.n_max) : 0;
  v.k1 = in.kp1 + (size_t)p * in.n_max * 3;
  v.k2 = in.kp2 + (size_t)p * in.n_max * 3;
  v.cp = in.corr ? in.corr + (size_t)p * in.n_max * 2 : nullptr;
  v.st = (r1 != v.m1 || r2 != v.m2 || rc != v.nc) ? EGONN_REG_STATUS_CLIPPED : 0;
  return v;
}

// |R s + tv - q|^2
__device__ static inline double pair_res2(const double* R, const double* tv, double sx, double sy, double sz, double qx, double qy,
                                          double qz) {
  const double dx = R[0] * sx + R[1] * sy + R[2] * sz + tv[0] - qx;
  const double dy = R[3] * sx + R[4] * sy + R[5] * sz + tv[1] - qy;
  const double dz = R[6] * sx + R[7] * sy + R[8] * sz + tv[2] - qz;
  return dx * dx + dy * dy + dz * dz;
}

// Lane t < nc: the points of correspondence t into c as fp64, c[0..2][t] = source x, y, z, c[3..5][t] = target.  Indices are
// clamped: nothing is read by an unchecked index.  Returns whether this lane's row held an index out of range.  No barrier.
template <int N>
__device__ static inline bool pair_load_corr(const float* __restrict__ k1, const float* __restrict__ k2, int m1, int m2,
                                             const int32_t* __restrict__ cp, int nc, double (*c)[N]) {
  const int t = threadIdx.x;
  bool bad = false;
  if (t < nc) {
    const int ci = cp[2 * t], cj = cp[2 * t + 1];
    bad = ci < 0 || ci >= m1 || cj < 0 || cj >= m2;
    const int i = clipi(ci, m1 - 1), j = clipi(cj, m2 - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c[k][t] = (double)k1[i * 3 + k];
      c[3 + k][t] = (double)k2[j * 3 + k];
    }
  }
  return bad;
}

// The same by the whole workgroup, ending in a barrier: the pair's status with BAD_INDEX and FEW_CORR decided.
template <int N>
__device__ static inline int pair_load_corr_status(const PairView& v, double (*c)[N]) {
  int st = v.st;
  if (__syncthreads_or(pair_load_corr(v.k1, v.k2, v.m1, v.m2, v.cp, v.nc, c))) st |= EGONN_REG_STATUS_BAD_INDEX;
  if (v.nc < 3) st |= EGONN_REG_STATUS_FEW_CORR;
  return st;
}

template <int NT>
struct PairTailShared {
  double q[3][NT];   // target keypoints, fp64
  double d2[NT];
  int nn[NT];
};

// The tail, by a workgroup of NT >= n_max lanes.  given: correspondences were given (else only repeatability is computed);
// model: (R row-major, tf) is an accepted model, else the caller passes the identity (Open3D returns the identity result when
// nothing beats fitness 0) and the pair ends with NO_MODEL and 0 inliers.  st: the status so far.
template <int NT>
__device__ static void pair_tail(const PairIn& in, const PairOut& o, int p, const PairView& v, bool given, bool model,
                                 const double* R, const double* tf, int st, PairTailShared<NT>& sh) {
  const int t = threadIdx.x, m1 = v.m1, m2 = v.m2;
  if (t < m2) {
#pragma unroll
    for (int k = 0; k < 3; ++k) sh.q[k][t] = (double)v.k2[t * 3 + k];
  }
  __syncthreads();
  double sx = 0.0, sy = 0.0, sz = 0.0;
  if (t < m1) sx = (double)v.k1[t * 3], sy = (double)v.k1[t * 3 + 1], sz = (double)v.k1[t * 3 + 2];

  if (given) {
    // final evaluation: every source keypoint under T, nearest target keypoint (ties: lowest index) closer than dist_th
    double bd = INFINITY;
    int bj = -1;
    if (t < m1 && model) {
      const double px = R[0] * sx + R[1] * sy + R[2] * sz + tf[0], py = R[3] * sx + R[4] * sy + R[5] * sz + tf[1],
                   pz = R[6] * sx + R[7] * sy + R[8] * sz + tf[2];
      for (int j = 0; j < m2; ++j) {
        const double dx = px - sh.q[0][j], dy = py - sh.q[1][j], dz = pz - sh.q[2][j];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 < bd) bd = d2, bj = j;
      }
    }
    sh.d2[t] = bd;
    sh.nn[t] = bj;
    __syncthreads();
    if (t == 0) {
      int k = 0;
      double e2 = 0.0;
      int32_t* cs = o.corr_set ? o.corr_set + (size_t)p * in.n_max * 2 : nullptr;
      for (int i = 0; i < m1; ++i)   // ascending i: a fixed summation order
        if (sh.nn[i] >= 0 && sh.d2[i] < in.th2) {
          if (cs) cs[2 * k] = i, cs[2 * k + 1] = sh.nn[i];
          e2 += sh.d2[i];
          ++k;
        }
      if (cs)
        for (int c = k; c < in.n_max; ++c) cs[2 * c] = cs[2 * c + 1] = -1;
      if (o.inliers) o.inliers[p] = k;
      if (o.fitness) o.fitness[p] = m1 > 0 ? (double)k / (double)m1 : 0.0;
      if (o.rmse) o.rmse[p] = k > 0 ? sqrt(e2 / (double)k) : 0.0;
      if (o.T) se3_store(R, tf, o.T + (size_t)p * 16);
    }
    if (!model) st |= EGONN_REG_STATUS_NO_MODEL;
  }

  if (in.T_gt) {
    const double* G = in.T_gt + (size_t)p * 16;
    // calculate_repeatability: share of source keypoints with a target keypoint within the threshold under T_gt (fp64)
    bool rep = false;
    if (t < m1) {
      const double px = G[0] * sx + G[1] * sy + G[2] * sz + G[3], py = G[4] * sx + G[5] * sy + G[6] * sz + G[7],
                   pz = G[8] * sx + G[9] * sy + G[10] * sz + G[11];
      double bd = INFINITY;
      for (int j = 0; j < m2; ++j) {
        const double dx = px - sh.q[0][j], dy = py - sh.q[1][j], dz = pz - sh.q[2][j];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 < bd) bd = d2;
      }
      rep = bd <= in.rth2;
    }
    const int nrep = __syncthreads_count(rep);
    if (t == 0) {
      if (o.repeatability) o.repeatability[p] = m1 > 0 ? (double)nrep / (double)m1 : 0.0;
      if (given) {
        const double dx = tf[0] - G[3], dy = tf[1] - G[7], dz = tf[2] - G[11];
        const double e_t = sqrt(dx * dx + dy * dy + dz * dz);
        double tr = 0.0;   // trace(R_est^T R_gt) = sum of the elementwise products
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) tr += R[r * 3 + c] * G[r * 4 + c];
        double cosv = (tr - 1.0) / 2.0;
        cosv = cosv < -1.0 ? -1.0 : (cosv > 1.0 ? 1.0 : cosv);
        const double e_r = acos(cosv) * 180.0 / 3.14159265358979323846;
        if (o.rte) o.rte[p] = e_t;
        if (o.rre) o.rre[p] = e_r;
        if (o.success) o.success[p] = (e_t > PAIR_RTE_MAX_M || e_r > PAIR_RRE_MAX_DEG) ? 0 : 1;
      }
    }
  }
  if (t == 0 && o.status) o.status[p] = st;
}

}  // namespace egonn
