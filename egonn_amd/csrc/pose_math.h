// Rigid-pose arithmetic in float64 shared by the pose graph (pose_graph.hip) and the loop-consistency filter
// (loop_consistency.hip): 3x3 algebra, SE(3) products as (R, t) pairs, the SO(3) logarithm and the validity test of an edge.
// Stated once here so that both files take the same logarithm (series threshold, atan2 form) and switch the same edges off.
// This header sets no contraction mode: its arithmetic is for those two files only.  se3_load and se3_store move data and
// nothing else, and are what the contraction-off code (pair_loop.h, pair_eval.h) takes from here.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/egonn_hip.h"

namespace egonn {

static constexpr double POSE_LOG_SMALL = 0.05;       // theta / sin(theta) by its series below this angle (pose_graph.hip, top)

// ------------------------------------------------------------------ small 3x3 algebra (row-major)
__device__ static inline void m3_mul(const double* A, const double* B, double* C) {            // C = A B
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ static inline void m3_tmul(const double* A, const double* B, double* C) {           // C = A^T B
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__device__ static inline void m3_mult(const double* A, const double* B, double* C) {           // C = A B^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}
__device__ static inline void m3_vec(const double* A, const double* x, double* y) {            // y = A x
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}
__device__ static inline void m3_tvec(const double* A, const double* x, double* y) {           // y = A^T x
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = A[i] * x[0] + A[3 + i] * x[1] + A[6 + i] * x[2];
}
__device__ static inline void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}

// ------------------------------------------------------------------ SE(3) as (R, t), R row-major
// the upper three rows of a (4,4) row-major pose
__device__ static inline void se3_load(const double* __restrict__ X, double* R, double* t) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = X[4 * i + j];
    t[i] = X[4 * i + 3];
  }
}
// (R, t) as a (4,4) row-major pose
__device__ static inline void se3_store(const double* R, const double* t, double* __restrict__ X) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) X[4 * i + j] = R[3 * i + j];
    X[4 * i + 3] = t[i];
  }
  X[12] = X[13] = X[14] = 0.0, X[15] = 1.0;
}
// (R, t) = A B
__device__ static inline void se3_mul(const double* Ra, const double* ta, const double* Rb, const double* tb, double* R, double* t) {
  m3_mul(Ra, Rb, R);
  m3_vec(Ra, tb, t);
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] += ta[i];
}
// (R, t) = A^-1 B, the difference of the translations taken first, so that offsets common to both cancel exactly
__device__ static inline void se3_inv_mul(const double* Ra, const double* ta, const double* Rb, const double* tb, double* R, double* t) {
  double d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = tb[i] - ta[i];
  m3_tmul(Ra, Rb, R);
  m3_tvec(Ra, d, t);
}
// (R, t) = A B^-1
__device__ static inline void se3_mul_inv(const double* Ra, const double* ta, const double* Rb, const double* tb, double* R, double* t) {
  double u[3];
  m3_mult(Ra, Rb, R);
  m3_vec(R, tb, u);
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = ta[i] - u[i];
}

// ------------------------------------------------------------------ Log_SO3
// the axial vector of R, its length sn = sin(theta), cs = cos(theta) from the trace; returns theta = atan2(sn, cs) in [0, pi],
// exact in both tails
__device__ static inline double so3_log_angle(const double* R, double* ax, double* sn, double* cs) {
  ax[0] = 0.5 * (R[7] - R[5]), ax[1] = 0.5 * (R[2] - R[6]), ax[2] = 0.5 * (R[3] - R[1]);
  *sn = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  *cs = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  return atan2(*sn, *cs);
}
// theta / sin(theta) below POSE_LOG_SMALL, truncated after theta^6
__device__ static inline double so3_log_series(double th2) {
  return 1.0 + th2 * (1.0 / 6.0 + th2 * (7.0 / 360.0 + th2 * (31.0 / 15120.0)));
}
// theta / sin(theta): Log R = ax * so3_log_scale(theta, theta^2, sn)
__device__ static inline double so3_log_scale(double th, double th2, double sn) {
  return th < POSE_LOG_SMALL ? so3_log_series(th2) : th / sn;
}

// ------------------------------------------------------------------ validity
// the plan's status bits of an edge (a, b, Z, (w_rot, w_trans)) over n poses; an edge with a bit set is off
__device__ static inline int pose_edge_status(int32_t a, int32_t b, int32_t n, const double* __restrict__ z, double wr, double wt) {
  int st = 0;
  if (a < 0 || a >= n || b < 0 || b >= n) st |= EGONN_PG_STATUS_BAD_INDEX;
  else if (a == b) st |= EGONN_PG_STATUS_SELF_LOOP;
  bool finite = fabs(wr) < INFINITY && fabs(wt) < INFINITY;              // false for NaN
#pragma unroll
  for (int j = 0; j < 12; ++j) finite = finite && fabs(z[j]) < INFINITY;
  finite = finite && z[12] == 0.0 && z[13] == 0.0 && z[14] == 0.0 && z[15] == 1.0;
  if (!finite) st |= EGONN_PG_STATUS_NONFINITE;
  if (wr < 0.0 || wt < 0.0) st |= EGONN_PG_STATUS_NEGATIVE_WEIGHT;
  return st;
}
// the upper three rows of a pose are finite
__device__ static inline bool pose_finite(const double* __restrict__ X) {
  bool finite = true;
#pragma unroll
  for (int j = 0; j < 12; ++j) finite = finite && fabs(X[j]) < INFINITY;
  return finite;
}
// the ranges of a graph that the plan's sort and its 32-bit indices hold
static inline bool pose_sizes_ok(int64_t n, int64_t E) { return n >= 1 && n < (1ll << 31) - 1 && E >= 0 && E < (1ll << 30); }

}  // namespace egonn
