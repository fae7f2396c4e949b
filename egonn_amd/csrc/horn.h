// Horn's closed form for the least-squares rotation between two centred point sets, shared by the ICP finish (icp.hip) and the
// spectral verification (spectral.hip): the unit quaternion is the largest eigenvector of a symmetric 4 x 4 matrix, found by
// cyclic Jacobi on a fixed schedule.  A unit quaternion is a proper rotation, so no reflection case exists.  Every operation is
// the IEEE operation that is written (contraction off), so both callers get the same bits from the same S.
#pragma once

#pragma clang fp contract(off)

namespace egonn {

// largest eigenvector of the symmetric 4 x 4 matrix A (cyclic Jacobi, fixed schedule): the unit quaternion (w, x, y, z)
__device__ static __forceinline__ void horn_top_eigenvector(double A[4][4], double* qv) {
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
  double top = A[0][0];   // the largest diagonal entry so far, kept in a register: A[m][m] would index A dynamically
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (A[i][i] > top) top = A[i][i], m = i;
  double nrm = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // column m of V, picked on the bit patterns: selects between loads become one dynamically indexed load, which would
    // keep V in scratch memory instead of registers
    uint64_t eb = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) eb |= __builtin_bit_cast(uint64_t, V[k][c]) & (m == c ? ~0ull : 0ull);
    const double e = __builtin_bit_cast(double, eb);
    qv[k] = e;
    nrm += e * e;
  }
  nrm = 1.0 / sqrt(nrm);
#pragma unroll
  for (int k = 0; k < 4; ++k) qv[k] *= nrm;
}

// R (row-major, det +1) maximising sum_k (R p_k) . q_k for S = sum_k p_k q_k^T of centred p, q
__device__ static inline void horn_rotation(const double S[3][3], double* U) {
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
  horn_top_eigenvector(N, qv);
  const double qw = qv[0], qx = qv[1], qy = qv[2], qz = qv[3];
  U[0] = 1.0 - 2.0 * (qy * qy + qz * qz), U[1] = 2.0 * (qx * qy - qw * qz), U[2] = 2.0 * (qx * qz + qw * qy);
  U[3] = 2.0 * (qx * qy + qw * qz), U[4] = 1.0 - 2.0 * (qx * qx + qz * qz), U[5] = 2.0 * (qy * qz - qw * qx);
  U[6] = 2.0 * (qx * qz - qw * qy), U[7] = 2.0 * (qy * qz + qw * qx), U[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
}

}  // namespace egonn
